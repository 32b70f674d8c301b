// RGCN block-diagonal gather-SpMM and its backward kernels for gfx950 (MI355X): what rgcn_csr.hip, rgcn_items.hip and
// rgcn_bwd.hip share -- chunk / relation-block primitives, the gathers' argument pack, raw-buffer and bf16 helpers, and the
// host front -- all in the anonymous namespace of the including translation unit (every family keeps its own kernels).
//
// Replaces, for RE-Net's RGCNBlockLayer (reference RGCN.py:79-94 + 42-50), the DGL/torch sequence
//   index_select(weight, type) [E, D*si]  ->  bmm (E*100 tiny GEMMs)  ->  fn.sum  ->  h*norm  -> +loop -> act
// with ONE pass: the destination row is the unit of work, the feature dimension lies across the
// lanes (float4 per lane: 50 lanes at D=200), the 1x1 / 2x2 / 4x4 relation block product is
// lane-local, the in-edges of the row are walked serially (rows are short: SURVEY 8, deg<=4 for
// 72-97 % of rows) so no cross-lane reduction and no atomics are needed, and the epilogue
// (norm, self-loop addend with dropout, ReLU) is fused.  HBM-bound integer/gather work: no MFMA.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int kWaves = 4;           // waves per workgroup
constexpr int kThreads = 64 * kWaves;

// Floats of a feature row that one lane owns per chunk.  SI = 1, 2, 4: a float4 (the relation blocks tile it).  SI = 3
// (D = 300): a 3x3 block does not tile a float4, so a lane owns exactly ONE block -- 3 features as a 12-byte load
// (dwordx3), its 9 block entries as three more -- 100 lanes in two chunks, the same lane / chunk geometry as D = 400.
// A chunk travels as a float4 whose .w is the constant 0 (no register).
template <int SI> constexpr int vw_of() { return SI == 3 ? 3 : 4; }
struct f32x3_mem { float x, y, z; };                    // 4-byte aligned: global_load / store_dwordx3

template <int VW>
__device__ __forceinline__ float4 ld_chunk(const float* base, size_t ch) {
    if constexpr (VW == 4) return reinterpret_cast<const float4*>(base)[ch];
    else {
        const f32x3_mem v = reinterpret_cast<const f32x3_mem*>(base)[ch];
        return make_float4(v.x, v.y, v.z, 0.f);
    }
}
template <int VW>
__device__ __forceinline__ void st_chunk(float* base, size_t ch, float4 o) {
    if constexpr (VW == 4) reinterpret_cast<float4*>(base)[ch] = o;
    else {
        f32x3_mem v; v.x = o.x; v.y = o.y; v.z = o.z;
        reinterpret_cast<f32x3_mem*>(base)[ch] = v;
    }
}
// dropout multipliers of chunk ch of row `row`.  The mask is defined on the float4 groups of the [rows, D] tensor
// (renet_drop4: group row * D/4 + f/4, element f % 4); a 3-float chunk straddles at most two of them.
template <int VW, int D>
__device__ __forceinline__ float4 drop_chunk(const DropCfg& d, uint64_t row, int ch) {
    if constexpr (VW == 4) return renet_drop4(d, row * (D / 4) + ch);
    else {
        if (d.thresh == 0) return make_float4(1.f, 1.f, 1.f, 1.f);
        const int f0 = 3 * ch, k0 = f0 & 3;
        const uint64_t g0 = row * (D / 4) + (f0 >> 2);
        const float4 a = renet_drop4(d, g0), b = renet_drop4(d, g0 + 1);       // (b unused when k0 <= 1)
        const float m[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float4 r;
        r.x = k0 == 0 ? m[0] : k0 == 1 ? m[1] : k0 == 2 ? m[2] : m[3];
        r.y = k0 == 0 ? m[1] : k0 == 1 ? m[2] : k0 == 2 ? m[3] : m[4];
        r.z = k0 == 0 ? m[2] : k0 == 1 ? m[3] : k0 == 2 ? m[4] : m[5];
        r.w = 0.f;
        return r;
    }
}

template <int SI, bool TR>
__device__ __forceinline__ void blockmul(const float4 x, const float4* __restrict__ w, float4& acc) {
    if constexpr (SI == 1) {
        const float4 w0 = w[0];
        acc.x = fmaf(x.x, w0.x, acc.x);
        acc.y = fmaf(x.y, w0.y, acc.y);
        acc.z = fmaf(x.z, w0.z, acc.z);
        acc.w = fmaf(x.w, w0.w, acc.w);
    } else if constexpr (SI == 2) {
        const float4 a = w[0], b = w[1];      // block0 = (a.x a.y ; a.z a.w)  block1 = (b.x b.y ; b.z b.w)
        if constexpr (!TR) {
            acc.x = fmaf(x.x, a.x, fmaf(x.y, a.z, acc.x));
            acc.y = fmaf(x.x, a.y, fmaf(x.y, a.w, acc.y));
            acc.z = fmaf(x.z, b.x, fmaf(x.w, b.z, acc.z));
            acc.w = fmaf(x.z, b.y, fmaf(x.w, b.w, acc.w));
        } else {
            acc.x = fmaf(x.x, a.x, fmaf(x.y, a.y, acc.x));
            acc.y = fmaf(x.x, a.z, fmaf(x.y, a.w, acc.y));
            acc.z = fmaf(x.z, b.x, fmaf(x.w, b.y, acc.z));
            acc.w = fmaf(x.z, b.z, fmaf(x.w, b.w, acc.w));
        }
    } else if constexpr (SI == 3) {
        const float4 r0 = w[0], r1 = w[1], r2 = w[2];              // rows i = 0..2 of the 3x3 block (xyz; w = 0)
        if constexpr (!TR) {
            acc.x = fmaf(x.x, r0.x, fmaf(x.y, r1.x, fmaf(x.z, r2.x, acc.x)));
            acc.y = fmaf(x.x, r0.y, fmaf(x.y, r1.y, fmaf(x.z, r2.y, acc.y)));
            acc.z = fmaf(x.x, r0.z, fmaf(x.y, r1.z, fmaf(x.z, r2.z, acc.z)));
        } else {
            acc.x = fmaf(x.x, r0.x, fmaf(x.y, r0.y, fmaf(x.z, r0.z, acc.x)));
            acc.y = fmaf(x.x, r1.x, fmaf(x.y, r1.y, fmaf(x.z, r1.z, acc.y)));
            acc.z = fmaf(x.x, r2.x, fmaf(x.y, r2.y, fmaf(x.z, r2.z, acc.z)));
        }
    } else {
        const float4 r0 = w[0], r1 = w[1], r2 = w[2], r3 = w[3];   // rows i = 0..3 of the 4x4 block
        if constexpr (!TR) {
            acc.x = fmaf(x.x, r0.x, fmaf(x.y, r1.x, fmaf(x.z, r2.x, fmaf(x.w, r3.x, acc.x))));
            acc.y = fmaf(x.x, r0.y, fmaf(x.y, r1.y, fmaf(x.z, r2.y, fmaf(x.w, r3.y, acc.y))));
            acc.z = fmaf(x.x, r0.z, fmaf(x.y, r1.z, fmaf(x.z, r2.z, fmaf(x.w, r3.z, acc.z))));
            acc.w = fmaf(x.x, r0.w, fmaf(x.y, r1.w, fmaf(x.z, r2.w, fmaf(x.w, r3.w, acc.w))));
        } else {
            acc.x = fmaf(x.x, r0.x, fmaf(x.y, r0.y, fmaf(x.z, r0.z, fmaf(x.w, r0.w, acc.x))));
            acc.y = fmaf(x.x, r1.x, fmaf(x.y, r1.y, fmaf(x.z, r1.z, fmaf(x.w, r1.w, acc.y))));
            acc.z = fmaf(x.x, r2.x, fmaf(x.y, r2.y, fmaf(x.z, r2.z, fmaf(x.w, r2.w, acc.z))));
            acc.w = fmaf(x.x, r3.x, fmaf(x.y, r3.y, fmaf(x.z, r3.z, fmaf(x.w, r3.w, acc.w))));
        }
    }
}

struct GatherArgs {
    const float* x;
    const int32_t* row_ptr;
    const int32_t* col;
    const int32_t* etype;
    const float* scale;
    const float* W;
    const float* addend;
    float* out;
    const int32_t* heavy;       // rows with in-degree > heavy_thresh, handled by rgcn_gather_heavy_kernel
    int n_heavy, heavy_thresh;
    int src_limit;              // edges whose source row is >= src_limit are skipped (pruned layer-2 backward)
    int addend_rows;            // rows >= addend_rows have no addend
    uint32_t x_rowb, w_rowb;    // item kernels: row stride in BYTES of x (fp32: 4 D; bf16: 2 ld) and of the relation table
    const int32_t* row_map;     // layer 1 on the entity table: addend row of output row v = row_map[v] (hub rows; the
                                // item stream carries it inside its flush items); nullptr = v
    int N, T, shift, relu;
    DropCfg drop;
};

// Buffer-descriptor loads (raw_buffer_load, hardware bounds check): an access past num_records returns 0 and
// touches no memory.  Every load of the item loop is therefore UNCONDITIONAL -- a skipped item, a lane beyond the
// feature row (lanes 50..63 at D = 200) or a flush item's relation block simply gets a descriptor with
// num_records = 0 / an offset past the row.  This matters more than it looks: with `if (valid) x = *p;` around the
// loads hipcc (ROCm 7.2) branches around each one and drains vmcnt at every merge point, i.e. the "UNR loads in
// flight" of the row-group kernel (rgcn_csr.hip) were in fact issued and waited for one at a time.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    // {base[31:0], base[47:32] (stride 0), num_records, dst_sel/format word of gfx9-family raw buffers}
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4s(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// Span of a whole-tensor descriptor and the "skip" vector offset.  The hardware compares the offset with
// num_records: whether or not the scalar (row) offset takes part in that comparison, kOob (+ row offset, no 32-bit
// wrap) is out of range and a valid lane's offset (+ row offset) in range as long as the tensor is smaller than
// 2 GiB; the entry points check that.
constexpr uint32_t kBufSpan = 0x80000000u;
constexpr uint32_t kOob = 0x80000000u;
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, uint32_t voff, float4 o) {
    u32x4 v;
    v.x = __float_as_uint(o.x); v.y = __float_as_uint(o.y); v.z = __float_as_uint(o.z); v.w = __float_as_uint(o.w);
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, 0, 0);
}

// chunk-width (VW floats) forms of the loads / the store: 16-byte, or 12-byte (dwordx3) with .w = 0
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
template <int VW>
__device__ __forceinline__ float4 buf_loadvs(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    if constexpr (VW == 4) return buf_load4s(r, voff, soff);
    else {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r, (int)voff, (int)soff, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), 0.f);
    }
}
template <int VW>
__device__ __forceinline__ void buf_storev(__amdgpu_buffer_rsrc_t r, uint32_t voff, float4 o) {
    if constexpr (VW == 4) buf_store4(r, voff, o);
    else {
        u32x3 v;
        v.x = __float_as_uint(o.x); v.y = __float_as_uint(o.y); v.z = __float_as_uint(o.z);
        __builtin_amdgcn_raw_buffer_store_b96(v, r, (int)voff, 0, 0);
    }
}

// bf16 STORAGE of the gather operands (BASELINE config 5; MX = 1: relation blocks bf16, MX = 2: source rows too):
// 8-byte loads of 4 bf16 per lane instead of 16-byte loads of 4 floats, widened to fp32 in registers (exact), fp32
// accumulation and fp32 addend / output as before.  At D = 400 the 6.4 KB relation block per edge is the stream that
// bounds the kernel: bf16 blocks halve it.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float4 buf_load4s_bf16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0);
    return make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
}

// ---- host front ---------------------------------------------------------------------------------------------------
// chunks per lane of a feature row: ceil(D / VW / 64) = 1, 1, 2, 2
template <int SI> constexpr int nch_of() { return (100 * SI / vw_of<SI>() + 63) / 64; }

// the run-time width as a template argument: f(std::integral_constant<int, SI>{}), SI = D / 100
template <class F>
int with_si(int D, F&& f) {
    switch (D) {
        case 100: return f(std::integral_constant<int, 1>{});
        case 200: return f(std::integral_constant<int, 2>{});
        case 300: return f(std::integral_constant<int, 3>{});
        case 400: return f(std::integral_constant<int, 4>{});
        default: return RENET_ERR_UNSUPPORTED;
    }
}

// the fields every gather entry sets the same way (heavy_thresh, and the item kernels' strides and row_map, are the
// entry's own); src_limit / addend_rows <= 0 = no limit
inline void gather_fill(GatherArgs& a, const float* x, const int32_t* row_ptr, const int32_t* col, const int32_t* etype,
                        const float* scale, const float* W, int T, int type_shift, const float* addend, float drop_p,
                        uint64_t seed, int relu, float* out, int N, const int32_t* heavy_rows, int n_heavy, int src_limit,
                        int addend_rows) {
    a.x = x; a.row_ptr = row_ptr; a.col = col; a.etype = etype; a.scale = scale; a.W = W;
    a.addend = addend; a.out = out; a.N = N; a.T = T; a.shift = type_shift; a.relu = relu;
    a.heavy = heavy_rows; a.n_heavy = n_heavy;
    a.src_limit = src_limit > 0 ? src_limit : 0x7fffffff;
    a.addend_rows = addend_rows > 0 ? addend_rows : 0x7fffffff;
    a.drop = make_drop(drop_p, seed);
}

// what every gather entry checks first, on the filled pack: the width, the hub-row list, then N / T / type_shift / drop_p
inline int gather_check(int D, const GatherArgs& a, float drop_p) {
    if (!renet_dim_ok(D)) return RENET_ERR_UNSUPPORTED;
    if (a.n_heavy < 0 || (a.n_heavy > 0 && !a.heavy)) return RENET_ERR_BADARG;
    if (a.N < 0 || a.T <= 0 || a.shift < 0 || a.shift >= a.T || drop_p < 0.f || drop_p >= 1.f) return RENET_ERR_BADARG;
    return RENET_OK;
}

}  // namespace
