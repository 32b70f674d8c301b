/*
 * renet_hip.h -- C ABI of librenet_hip.so: the MI355X (gfx950) kernels behind RE-Net's
 * RENet / RGCNAggregator Python API.
 *
 * The reference (INK-USC/RE-Net) has NO native code and NO FFI: its boundary for this path is the
 * Python class API (RGCN.py, Aggregator.py, model.py, global_model.py) and everything below that is
 * third-party (DGL 0.4 + torch 1.6 CUDA kernels).  Each entry point below therefore names the
 * reference lines whose device work it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm tensors: tensor.data_ptr());
 *     the library allocates nothing and keeps no global mutable state (re-entrant);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); every
 *     call only enqueues work on it and never synchronises;
 *   - fp32 row-major contiguous matrices, int32 indices;
 *   - D (n_hidden) must be 100, 200, 300 or 400 (the reference hard-codes num_bases = 100, model.py:36,
 *     so the relation blocks are 1x1, 2x2, 3x3, 4x4); other values return RENET_ERR_UNSUPPORTED, and so
 *     do the bf16-storage entries (renet_rgcn_gather_items*_bf16, renet_gru_*_layouts_bf16*) at D = 300;
 *   - return value: 0 = ok, <0 = argument error (below), >0 = hipError_t from the launch.
 */
#ifndef RENET_HIP_H
#define RENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RENET_OK 0
#define RENET_ERR_BADARG (-1)
#define RENET_ERR_UNSUPPORTED (-2)
#define RENET_ERR_WORKSPACE (-3)

#define RENET_ABI_VERSION 1
int renet_version(void);

/* ------------------------------------------------------------------------------------------------
 * Row gather / deterministic segmented scatter-add.
 * renet_gather_rows : out[i,:] = table[idx[i],:]              (utils.py:239 h0 = ent_embeds[id];
 *                                                              Aggregator.py:139-140 subject rows)
 * renet_segment_add : for u in [0,U): dst[seg_target[u],:] += sum_{k in [seg_ptr[u],seg_ptr[u+1])}
 *                     src[order[k],:]   -- the backward of renet_gather_rows with the index sorted on
 *                     the host (no atomics => bit-reproducible).
 * ---------------------------------------------------------------------------------------------- */
int renet_gather_rows(const float* table, const int32_t* idx, int n, int D, float* out, void* stream);
int renet_segment_add(const float* src, const int32_t* order, const int32_t* seg_ptr,
                      const int32_t* seg_target, int U, int D, float* dst, void* stream);
/* Two segmented adds that share ONE plan in one launch: dst0[target[u]] += sum of src0 rows, dst1[target[u]] += sum
 * of src1 rows (the first RGCN layer's backward reduces both the message gradient and the self-loop gradient of the
 * batch graph's nodes to entity rows, keyed by the same node -> entity map). */
int renet_segment_add2(const float* src0, const float* src1, const int32_t* order, const int32_t* seg_ptr,
                       const int32_t* seg_target, int U, int D, float* dst0, float* dst1, void* stream);
/* Up to RENET_SEGADD_MAX_JOBS independent segmented adds in ONE launch, each with up to two stages over its plan:
 *   stage A:            dst[target[u]] = dst[target[u]] + sum_seg (a0[row] (+ a1[row]))     (a1 optional)
 *   stage B (optional): dst[target[u]] = that           + sum_seg  b[row]
 * Per segment and stage the additions are renet_segment_add's, in its order, so a job equals renet_add_inplace(a0, a1)
 * followed by renet_segment_add(a0) and renet_segment_add(b) bit for bit (a0 + a1 is formed as the rows are loaded; a0 is
 * not modified).  overwrite != 0: stage A starts from 0.f instead of the old row (dst[t] = 0.f + sum: what renet_zero
 * followed by the add leaves, also for an empty segment and for a sum of -0.0 terms); accepted only where the plan covers
 * every row of dst: U == dst_rows (targets are distinct by the plan's contract).  Refused before any launch: n out of
 * range, a missing array, an overwrite job with U != dst_rows, two jobs with the same dst (RENET_ERR_BADARG); D > 512
 * (RENET_ERR_UNSUPPORTED).  Jobs with U == 0 are no-ops. */
#define RENET_SEGADD_MAX_JOBS 4
typedef struct {
    const int32_t *order, *seg_ptr, *seg_target;
    int U;                                     /* segments of the plan */
    float* dst;
    int dst_rows;                              /* rows of dst (read for overwrite jobs only) */
    int overwrite;
    const float *a0, *a1, *b;                  /* a1, b: optional */
} RenetSegAddJob;
int renet_segment_add_multi(int n, const RenetSegAddJob* jobs, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RGCN block-diagonal gather-SpMM  (RGCN.py:79-94 msg_func + fn.sum + apply_func, fused with the
 * epilogue of RGCN.py:42-50).
 *
 *   out[v,:] = act( scale[v] * sum_{e in [row_ptr[v],row_ptr[v+1])} blockmul(x[col[e],:], W[tau(e)])
 *                   + addend[v,:] * dropmask )
 *   tau(e)   = (etype[e] + type_shift) mod T                       (T = 2 * num_rels)
 *   blockmul : x viewed [nb=100, si], W[tau] viewed [nb, si, so] row-major (RGCN.py:81-87):
 *              transpose_w == 0: y[b,j] = sum_i x[b,i] W[b,i,j]     (forward message)
 *              transpose_w == 1: y[b,i] = sum_j x[b,j] W[b,i,j]     (backward wrt h through W^T)
 *   scale    : per-destination 1/in-degree (`norm`, utils.py:126-127) or NULL (= 1)
 *   addend   : the self-loop message h @ W_loop (RGCN.py:34-37) or NULL; may alias `out`.
 *              drop_p > 0 applies inverted dropout to the addend with the counter-based mask
 *              keep(seed, v*D+c) (RGCN.py:36-37); the same (seed) regenerates the mask in backward.
 *   relu     : 1 = ReLU epilogue (rgcn1, Aggregator.py:119-120), 0 = identity (rgcn2)
 *
 * The graph is CSR by destination (row_ptr[N+1], col[E] = source row, etype[E]).
 * heavy_rows[n_heavy] (optional, may be NULL/0) lists the rows whose in-degree exceeds heavy_thresh:
 * the row-group kernel skips them and a second launch reduces each with a whole workgroup, so a
 * Zipf-tail hub row cannot serialise one wave for the entire launch.
 * src_limit > 0 skips edges whose source row is >= src_limit and addend_rows > 0 restricts the addend to
 * rows < addend_rows (0 = no restriction): used by the backward of a layer that was only evaluated on a
 * prefix of the rows (RE-Net reads the second RGCN layer only at the subject rows, Aggregator.py:139-140).
 * The backward wrt x uses the same CSR: RE-Net graphs hold both directions of every fact with paired
 * types (utils.py:74-76), so the transposed graph is the same structure with type_shift = num_rels.
 * ---------------------------------------------------------------------------------------------- */
int renet_rgcn_gather(const float* x, int D, const int32_t* row_ptr, const int32_t* col,
                      const int32_t* etype, const float* scale, const float* W, int T, int type_shift,
                      int transpose_w, const float* addend, float drop_p, uint64_t seed, int relu,
                      float* out, int N, const int32_t* heavy_rows, int n_heavy, int heavy_thresh,
                      int src_limit, int addend_rows, void* stream);

/* The same operator on the planned ITEM STREAM of the graph (the production path; renet_rgcn_gather above needs no
 * plan and stays as the plain-CSR entry).  The host planner (renet_host_gather_items / graph.plan_gather_items)
 * linearises every LIGHT row (in-degree <= heavy) as its in-edges (it_src = source row, it_type = type_s) followed
 * by a flush item (it_src = the row, it_type = -1) and cuts the stream into n_groups groups of <= 64 items
 * (grp_ptr[n_groups + 1]); one wave takes one group, all of its loads are unconditional buffer loads UNR items at a
 * time (the self-loop addend and norm of a row are loaded by its flush item like any edge's operands), hub rows
 * (heavy_rows[n_heavy], in-degree > heavy, NOT in the stream) are reduced by one workgroup each in the same
 * launch.  row_ptr / col / etype are only read for hub rows.  pruned != 0 only selects the kernel NAME
 * (rgcn_gather_{fwd,bwdh}_{full,pruned}: a kernel trace separates the four launch classes of a training step);
 * the caller passes the group / hub-row prefix that covers rows < N.  x, addend, out, W must each be smaller than 2 GiB (32-bit buffer offsets).
 * Replaces RGCN.py:79-94 + 42-50 exactly as renet_rgcn_gather does. */
int renet_rgcn_gather_items(const float* x, int D, const int32_t* it_src, const int32_t* it_type,
                            const int32_t* grp_ptr, int n_groups, const int32_t* row_ptr, const int32_t* col,
                            const int32_t* etype, const float* scale, const float* W, int T, int type_shift,
                            int transpose_w, const float* addend, float drop_p, uint64_t seed, int relu,
                            float* out, int N, const int32_t* heavy_rows, int n_heavy, int src_limit,
                            int addend_rows, int pruned, void* stream);

/* The FIRST RGCN layer addressed through the entity table (utils.py:239 + RGCN.py:35,79-94): the reference
 * materialises h0 = ent_embeds[id] ([N, D], one row per node of the batch graph) and multiplies it by W_loop; since
 * h0 @ W_loop == (ent_embeds @ W_loop)[id], the layer can read BOTH its source rows and its self-loop addend from
 * [table_rows, D] tables (ent_embeds and ent_embeds @ W_loop, computed once per step on N_ent rows instead of N):
 *   out[v] = act( scale[v] * sum_{e=(u->v)} blockmul(table[row_map[u]], W[type_e]) + drop(addend_table[row_map[v]]) )
 * it_src_t / it_type_t / col_t are the item stream / CSR columns with the source rows already composed through
 * row_map (renet_compose_table_items); flush items carry row_map[v] inside it_type (-3 - row_map[v]).  Forward
 * only (the backward pass of the layer is the ordinary transposed gather on [N, D] gradients). */
int renet_rgcn_gather_items_table(const float* table, int table_rows, int D, const int32_t* it_src_t,
                                  const int32_t* it_type_t, const int32_t* grp_ptr, int n_groups,
                                  const int32_t* row_ptr, const int32_t* col_t, const int32_t* etype,
                                  const int32_t* row_map, const float* scale, const float* W, int T, int type_shift,
                                  const float* addend_table, float drop_p, uint64_t seed, int relu, float* out, int N,
                                  const int32_t* heavy_rows, int n_heavy, void* stream);

/* bf16-STORAGE forms of the two item-stream gathers (BASELINE config 5, bench.py --dtype bf16): the relation-block
 * table W_bf16 [T, w_ld] (row stride w_ld >= D * D/100 bf16 elements; a renet_pack_bf16 matrix) and -- table form --
 * the entity table table_bf16 [table_rows, table_ld] are read as bf16 and widened in registers; x / the gradient rows,
 * the addend and the output stay fp32, accumulation is fp32.  Same arguments and results otherwise (the product
 * rounds W / the table to bf16 exactly as the bf16 GEMMs of this mode do with their operands).
 * Replaces, like the fp32 forms: RGCN.py:53-77,79-94 (msg_func / bmm + fn.sum + apply_func). */
int renet_rgcn_gather_items_bf16(const float* x, int D, const int32_t* it_src, const int32_t* it_type,
                                 const int32_t* grp_ptr, int n_groups, const int32_t* row_ptr, const int32_t* col,
                                 const int32_t* etype, const float* scale, const void* W_bf16, int w_ld, int T,
                                 int type_shift, int transpose_w, const float* addend, float drop_p, uint64_t seed,
                                 int relu, float* out, int N, const int32_t* heavy_rows, int n_heavy, int src_limit,
                                 int addend_rows, int pruned, void* stream);
int renet_rgcn_gather_items_table_bf16(const void* table_bf16, int table_ld, int table_rows, int D,
                                       const int32_t* it_src_t, const int32_t* it_type_t, const int32_t* grp_ptr,
                                       int n_groups, const int32_t* row_ptr, const int32_t* col_t, const int32_t* etype,
                                       const int32_t* row_map, const float* scale, const void* W_bf16, int w_ld, int T,
                                       int type_shift, const float* addend_table, float drop_p, uint64_t seed, int relu,
                                       float* out, int N, const int32_t* heavy_rows, int n_heavy, void* stream);
/* Composes the per-batch index arrays of the table-addressed layer on the device (once per batch):
 * it_src_t / it_type_t [n_items], col_t [E] (CSR columns), e_src_t [E] (relation-bucketed edge list of
 * renet_rgcn_bwd_w) = the plain arrays with every SOURCE row u replaced by row_map[u]. */
int renet_compose_table_items(const int32_t* row_map, const int32_t* it_src, const int32_t* it_type, int n_items,
                              const int32_t* col, const int32_t* e_src, int E, int32_t* it_src_t,
                              int32_t* it_type_t, int32_t* col_t, int32_t* e_src_t, void* stream);

/* Backward prologue of one RGCN layer (element-wise, RGCN.py:42-50 + :93-94 reversed):
 *   g_pre = g_out * (relu ? out > 0 : 1);  gn = g_pre * norm[v];  g_loop = g_pre * dropmask       */
int renet_rgcn_bwd_prep(const float* g_out, const float* out, const float* norm, int relu,
                        float drop_p, uint64_t seed, int N, int D, float* gn, float* g_loop,
                        void* stream);
/* The same with the operand bound of g_loop for renet_gemm_f32_h3: bound_part receives renet_bound_parts(N * D / 4)
 * floats (one maximum of |g_loop| per workgroup). */
int renet_rgcn_bwd_prep_bounds(const float* g_out, const float* out, const float* norm, int relu,
                               float drop_p, uint64_t seed, int N, int D, float* gn, float* g_loop,
                               float* bound_part, void* stream);

/* Gradient of the relation weights (RGCN.py:81-87 backward):
 *   dW[tau, b, i, j] = sum_{e: tau(e) == tau} x[src[e], b*si+i] * gn[dst[e], b*so+j]
 * Edges are pre-sorted by type and cut into chunks of one type each (host side):
 *   chunk c covers sorted edges [chunk_ptr[c], chunk_ptr[c+1]) , all of type chunk_type[c];
 *   type_chunk_ptr[T+1] lists, per type, its range of chunks; the stored type t accumulates into
 *   dW[(t + type_shift) mod T] (same convention as renet_rgcn_gather).  Two deterministic passes:
 *   per-chunk partial sums into `workspace` (n_chunks * D*D/100 floats), then a per-type reduction.
 *   A chunk may hold any number of edges: the planners cut at 64 (graph.CHUNK, the `chunk` argument of
 *   renet_host_type_chunks), the kernel walks a chunk 64 edges at a time and sets no upper limit, and an EMPTY chunk
 *   (chunk_ptr[c] == chunk_ptr[c+1]) contributes nothing, wherever it stands in its type.  A type without chunks gets
 *   dW[tau] = beta * dW[tau]; with n_chunks == 0 that is all the call does (chunk_ptr / chunk_type are not read).
 *   `workspace` need not be initialised (tests/test_gpu_reductions.py runs all of this on a NaN-filled workspace of
 *   exactly renet_rgcn_bwd_w_workspace bytes).
 *   x and gn must each be smaller than 2 GiB (rows are addressed with 32-bit buffer offsets). */
size_t renet_rgcn_bwd_w_workspace(int n_chunks, int D);
int renet_rgcn_bwd_w(const float* x, const float* gn, const int32_t* e_src, const int32_t* e_dst,
                     const int32_t* chunk_ptr, const int32_t* chunk_type, int n_chunks,
                     const int32_t* type_chunk_ptr, int T, int type_shift, int D, float* dW, float beta,
                     float* workspace, size_t workspace_bytes, void* stream);
/* The same with 64-bit global addressing of the rows of x / gn: for feature tensors of 2 GiB and more, which the
 * 32-bit buffer offsets of renet_rgcn_bwd_w cannot reach (the counterpart of renet_rgcn_gather for the gather entry). */
int renet_rgcn_bwd_w64(const float* x, const float* gn, const int32_t* e_src, const int32_t* e_dst,
                       const int32_t* chunk_ptr, const int32_t* chunk_type, int n_chunks,
                       const int32_t* type_chunk_ptr, int T, int type_shift, int D, float* dW, float beta,
                       float* workspace, size_t workspace_bytes, void* stream);   /* dW = beta * dW + ... */

/* ------------------------------------------------------------------------------------------------
 * fp32 GEMM on the f32-input MFMA (exact fp32, v_mfma_f32_32x32x2_f32):
 *   C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] (+ bias[N]) (+ beta * C)
 *   ta == 0: A is [M,K] row-major (lda = K-stride);  ta == 1: A is stored [K,M] (A^T)
 *   tb == 0: B is [K,N] row-major;                    tb == 1: B is stored [N,K] (B^T)
 * Replaces torch.mm (RGCN.py:35), the GRU input projection inside nn.GRU (model.py:86,94), nn.Linear
 * (model.py:89-90,98-99) and their autograd backward GEMMs.
 * split_k > 1 runs the deterministic two-pass split-K (partials in `workspace`,
 * renet_gemm_workspace bytes) for the tall-skinny weight-gradient shapes.
 * Products are EXACT fp32 (no operand rounding: integer-valued operands give integer-exact results), accumulation is
 * fp32 in a fixed k order.  Since round 4 the kernel addresses its operands through raw buffer descriptors (32-bit byte
 * offsets, branch-free k-loop; csrc/gemm.hip); operands it cannot reach that way (>= 4 GiB) run the round-1 kernel
 * with 64-bit addressing -- same contract, same results up to summation order.
 * ---------------------------------------------------------------------------------------------- */
size_t renet_gemm_workspace(int M, int N, int split_k);
int renet_gemm_f32(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                   const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                   int split_k, float* workspace, size_t workspace_bytes, void* stream);

/* Same contract as renet_gemm_f32, computed on the bf16 matrix cores with every fp32 operand split into
 * three bf16 terms and the six leading term products accumulated in fp32 ("bf16x6"): fp32-class accuracy
 * (dropped terms <= 2^-23 relative) at 16/6 of the f32-input MFMA rate.  See csrc/gemm_split.hip. */
int renet_gemm_f32_split(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                         const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                         int split_k, float* workspace, size_t workspace_bytes, void* stream);

/* What renet_gemm_f32_split launches for a problem -- the launcher executes exactly this plan (csrc/gemm_split.hip,
 * plan_split); pure host logic, callable without a GPU.  A / B may be NULL (only their 16-byte alignment is looked at,
 * for the weight-resident kernel).  plan[8] (host ints):
 *   [0] kernel: 0 fused k-loop (one workgroup per CU; grids of <= 256 tiles), 1 two-phase 128 x 128 tiles, 2 two-phase
 *       256 x 128 tiles, 3 weight-resident kernel (N <= 256, K <= 208, gemm_skinny.hip)
 *   [1] two-phase kernels: 1 = operands through raw buffer descriptors (both reach < 2^30 elements), 0 = 64-bit loader
 *   [2] tile order: 0 plain (blockIdx.x, blockIdx.y); w >= 1: XCD-aware order with panels of <= w tiles (8 by default,
 *       narrowed per shape for un-split grids whose short operand does not fit an L2; split-K grids map whole k-slices to
 *       one XCD)
 *   [3..5] grid (x = column tiles, y = row tiles, z = k-slices)   [6] the split factor after clamping   [7] 0 */
int renet_gemm_split_plan(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                          int split_k, int* plan);

/* Same contract as renet_gemm_f32 on the f16 matrix cores ("f16x3", csrc/gemm_h3.h): every operand value, scaled by
 * a power of two of its tensor so that max |x| lands in [2^14, 2^15), is split into two binary16 terms
 * x s = h1 + 2^-11 h2 (22 significant bits) and a b is evaluated as a1 b1 + 2^-11 (a1 b2 + a2 b1) with fp32
 * accumulation: split error and dropped term are each <= 2^-22 relative for every element with |x| >= 2^-29 max |x|
 * (smaller elements keep an ABSOLUTE error <= 2^-39 max |x|), unbiased, so that a K-long dot product stays within a
 * small multiple of the error of fp32 products with fp32 accumulation (measured next to renet_gemm_f32 and
 * renet_gemm_f32_split in tests/test_gpu_parity.py) -- with three matrix instructions per fragment pair
 * instead of six.  maxA / maxB: nA / nB (1..1024) device floats whose largest magnitude bounds max |A| / max |B|
 * from above -- the output of renet_maxabs_partials, or any bound the caller knows (a bound 2^k too large costs k of
 * the 29 binades).  A bound that is too SMALL overflows binary16: undefined results (inf / NaN).
 *   renet_maxabs_partials : part[b], b < renet_maxabs_blocks(rows, cols, ld) <= 256 (part[0] = 0 for an empty matrix):
 *                           the maxima of |x| over disjoint parts of x[rows, cols] (row stride ld); NaNs are ignored.
 * Replaces the same reference calls as renet_gemm_f32 (torch.mm RGCN.py:35, nn.GRU's input projection model.py:86,94,
 * nn.Linear model.py:89-90,98-99 and their backward GEMMs). */
int renet_maxabs_blocks(int rows, int cols, int ld);
int renet_maxabs_partials(const float* x, int rows, int cols, int ld, float* part, void* stream);
/* renet_maxabs_partials for n_jobs CONTIGUOUS, 16-byte aligned arrays in one launch (a model's weights, once per
 * optimizer step).  jobs: device array of n_jobs records {const float* x; uint64 n4 (number of float4); float* part;
 * int32 nblocks (<= 256 partials written to part); int32 pad}. */
int renet_maxabs_partials_multi(const void* jobs, int n_jobs, void* stream);
int renet_gemm_f32_h3(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B,
                      int ldb, float beta, float* C, int ldc, const float* bias, int split_k, float* workspace,
                      size_t workspace_bytes, const float* maxA, int nA, const float* maxB, int nB, void* stream);

/* Same contract in bf16 mixed precision (BASELINE config 5: "n_hidden=400 bf16"): every fp32 operand value is
 * rounded to bf16 (RNE) on its way into LDS, products on v_mfma_f32_32x32x16_bf16, fp32 accumulation, fp32 C.
 * Relative error of a product ~2^-8 per operand; a K-long dot product of O(1) terms is accurate to ~2^-8/sqrt(K)
 * relative to its magnitude scale (tolerances: tests/test_gpu_bf16.py). */
int renet_gemm_bf16(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                    const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
                    int split_k, float* workspace, size_t workspace_bytes, void* stream);

/* bf16 STORAGE (BASELINE config 5, "n_hidden=400 bf16"): operands live in HBM as bf16 matrices, [Rp][Cp] row-major
 * with Rp, Cp = R, C rounded up to multiples of 256 and zero padding.
 *   renet_pack_bf16  : fp32 X[R, C] (row stride ldx) -> bf16 (RNE), padding written; renet_bf16_bytes(R, C) bytes.
 *   renet_gemm_bf16s : C[M,N] = alpha * op(A) op(B) (+ bias) (+ beta * C) on such matrices, contraction length K: ONE bf16
 *                      product per element pair (v_mfma_f32_32x32x16_bf16), fp32 accumulation, fp32 C; operands staged by
 *                      LDS-DMA (global_load_lds) through a 3-deep LDS ring.
 *       a_tr == 0: A is stored as [M rows][K cols] (K contiguous);  a_tr == 1: A^T, i.e. [K rows][M cols] (the tensor as
 *                  stored when the contraction runs over its rows): fragments come from ds_read_b64_tr_b16
 *       b_tr == 0: B^T as [N rows][K cols] (nn.Linear's weight layout);  b_tr == 1: B as [K][N]
 *     One stored matrix serves both roles: linear.weight [N_ent, 3D] is op(B) of the logits GEMM (b_tr = 0) and of
 *     dfeat = dlogits W (b_tr = 1); dlogits [B, N_ent] is op(A) of dfeat (a_tr = 0) and of dW = dlogits^T feat (a_tr = 1).
 *     split_k / workspace as renet_gemm_f32.  Replaces torch.mm / nn.Linear /
 *                      nn.GRU's input projection at config 5 (RGCN.py:35, model.py:86-99) -- the reference itself
 *                      has no bf16 path; tolerances in tests/test_gpu_bf16.py. */
size_t renet_bf16_bytes(int R, int C);
int renet_pack_bf16(const float* X, int R, int C, int ldx, void* out, void* stream);
int renet_gemm_bf16s(int a_tr, int b_tr, int M, int N, int K, float alpha, const void* Ap, int lda, const void* Bp,
                     int ldb, float beta, float* C, int ldc, const float* bias, int split_k, float* workspace,
                     size_t workspace_bytes, void* stream);
/* Producers that write the bf16 operand format directly (no fp32 copy of the tensor exists in bf16 mode).  A
 * bf16-storage GEMM reads the contraction dimension in 64-wide stages, so the padding a consumer may touch --
 * columns [C, ceil64(C)) of the valid rows and rows [rows, ceil64(rows)) -- must be zero: each producer below zeroes
 * it, renet_bf16_zero_padding does so for a buffer filled by some other kernel.
 *   renet_seq_assemble_fwd_bf16   : renet_seq_assemble_fwd with X [S, 4D] / Xr [S, 3D] as bf16, row strides ldx / ldxr
 *   renet_softmax_ce_bf16         : renet_softmax_ce with the gradient (softmax - onehot) * grad_scale as bf16 (the
 *                                   fp32 logits are left untouched)
 *   renet_gru_bwd_layouts_bf16out : renet_gru_bwd_layouts_bf16 with dGi / dGh [S, 3H] as bf16, row stride out_ld
 *   renet_colsum_bf16 / renet_scale_bf16_by_device_scalar : the bias-gradient column sums / upstream-gradient scaling
 *                                   on such matrices */
int renet_bf16_zero_padding(void* P, int rows, int C, int ld, int rows_alloc, void* stream);
int renet_seq_assemble_fwd_bf16(const float* h2, const float* ent, const float* rel, const float* glob,
                                const int32_t* subj_row, const int32_t* row_ent, const int32_t* row_rel,
                                const int32_t* glob_row, int S, int D, float drop_p, uint64_t seed_x,
                                uint64_t seed_xr, void* X, int ldx, void* Xr, int ldxr, int rows_alloc,
                                void* stream);
int renet_softmax_ce_bf16(const float* logits, const int32_t* target, int B, int C, int ld, float grad_scale,
                          float* row_loss, void* dlogits_bf16, int ld16, int rows16, void* stream);
int renet_gru_bwd_layouts_bf16out(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L,
                                  int H, const float* const* Whh, const float* const* saved, void* const* dGi16,
                                  void* const* dGh16, int out_ld, float* workspace, size_t workspace_bytes,
                                  void* stream);
int renet_colsum_bf16(const void* X, int M, int N, int ldx, float* out, float beta, float* workspace,
                      size_t workspace_bytes, void* stream);
int renet_scale_bf16_by_device_scalar(void* x, size_t n, const float* scale, void* stream);

/* PLANES (round 6): the bf16x6 arithmetic of renet_gemm_f32_split on operands that are ALREADY split -- a matrix [R, C] is
 * stored as three bf16 matrices ("planes", x = p1 + p2 + p3, p1 = rne(x), p2 = rne(x - p1), p3 = rne(x - p1 - p2): the
 * split the bf16x6 loaders perform per k-tile), each over the padded extent [Rp][Cp] (R, C rounded up to multiples of 256,
 * ZERO padding), `plane` elements apart.  Inside a plane the elements are TILED, not row-major ("T16": 16 x 16 tiles of
 * 512 bytes, tile (tr, tc) at (tr * Cp / 16 + tc) * 256 elements; element (i, j) of a tile at
 * (i ^ 4 * (tc & 1)) * 16 + ((j >> 3) ^ ((i >> 3) & 1)) * 8 + (j & 7) -- csrc/common.h renet_t16_off): every 1 KB
 * LDS-DMA piece of the GEMM is then two whole tiles whether the matrix is contracted over its columns or over its rows,
 * and both kinds of fragment read are free of LDS bank conflicts (tools/p6_layout_sim.py models the data path).
 * The producers write the format directly (renet_softmax_ce_planes: the CE gradient; renet_pack_planes: anything
 * else -- a weight once per optimizer step), so the GEMM k-loop contains no conversion: LDS-DMA staging
 * (global_load_lds) into a 3-slot ring of 128 x 128 x 16 half-stages (two workgroups per CU; RENET_P6_TILE=256: 4 slots of
 * 256 x 128 x 16, one workgroup per CU), fragments double buffered in registers, six
 * v_mfma_f32_32x32x16_bf16 per fragment pair, fp32 accumulation; same result as renet_gemm_f32_split up to fp32
 * summation order.
 *   renet_planes_elems : Rp * Cp, the element count of one plane (the plane stride the packers use)
 *   renet_pack_planes  : fp32 X[R, C] (row stride ldx) -> planes; ones_col != 0 appends a column of ones (C + 1 columns:
 *                        see col_out)
 *   renet_gemm_planes  : C[M, N] = alpha * (*alpha_dev) * op(A) op(B) (+ bias) (+ beta * C);  lda / ldb = Cp of the
 *                        stored matrices
 *       a_tr == 0: A stored [M rows][K cols];  a_tr == 1: stored [K rows][M cols] (contraction over its rows)
 *       b_tr == 0: B^T stored [N rows][K cols] (nn.Linear's weight layout);  b_tr == 1: B stored [K rows][N cols]
 *       alpha_dev : optional DEVICE scalar folded into alpha (the upstream autograd gradient: no pass over the operand)
 *       col_out   : optional; N then counts one EXTRA logical column whose values go to col_out[M] instead of C -- with
 *                   B packed with ones_col this is the bias gradient sum_k op(A)[m, k] inside the weight-gradient GEMM
 *       split_k / workspace as renet_gemm_f32 (renet_gemm_workspace(M, N, split_k) with this N).
 * Replaces nn.Linear's forward and backward GEMMs of the entity score head (model.py:89-90 and autograd), like
 * renet_gemm_f32_split. */
size_t renet_planes_elems(int R, int C);
int renet_pack_planes(const float* X, int R, int C, int ldx, int ones_col, void* out, void* stream);
int renet_gemm_planes(int a_tr, int b_tr, int M, int N, int K, float alpha, const float* alpha_dev, const void* Ap,
                      int lda, size_t a_plane, const void* Bp, int ldb, size_t b_plane, float beta, float* C, int ldc,
                      const float* bias, float* col_out, int split_k, float* workspace, size_t workspace_bytes,
                      void* stream);
/* renet_softmax_ce with the gradient (softmax - onehot) * grad_scale written as T16 planes over [rows16][ld16] (`plane`
 * elements apart; ld16 % 16 == 0, rows16 >= ceil16(B); columns [C, ld16) of the rows < B and the rows [B, ceil16(B))
 * zeroed); the fp32 logits are left untouched.
 * Replaces F.cross_entropy's backward (model.py:91,100) as renet_softmax_ce does. */
int renet_softmax_ce_planes(const float* logits, const int32_t* target, int B, int C, int ld, float grad_scale,
                            float* row_loss, void* dl_planes, size_t plane, int ld16, int rows16, void* stream);
/* renet_softmax_ce_planes for the loss THROUGH THE COPY MIX (renet_mix_ce below states it): the same planes -- T16 layout,
 * three-term RNE split, zeroed columns [C, ld16) and rows [B, ceil16(B)), the same row-to-workgroup map, the logits left
 * untouched -- of (softmax - onehot) * (grad_scale * s_b), with row_loss and d_a as there.  The four-row writer for aligned
 * C >= 2048 (ld16 <= 24576), the generic writer otherwise; RENET_SOFTMAX_ROWS is not read.  a_row = 0 gives the planes and
 * losses of renet_softmax_ce_planes bit for bit.  A missing array, ld < C or a planes buffer that does not fit:
 * RENET_ERR_BADARG before any launch. */
int renet_mix_ce_planes(const float* logits, const int32_t* target, const float* a_row, const float* q_row, int B, int C,
                        int ld, float grad_scale, float* row_loss, void* dl_planes, size_t plane, int ld16, int rows16,
                        float* d_a, void* stream);
/* renet_mix_ce_planes for the loss through the JOINT mix (renet_joint_mix_ce below states it): lp_row[b] is added to the gold
 * logit, s_row (optional) receives s_b; planes, padding, row map and refusals as renet_mix_ce_planes, and a missing lp_row.
 * lp_row = 0 gives renet_mix_ce_planes bit for bit. */
int renet_joint_mix_ce_planes(const float* logits, const int32_t* target, const float* a_row, const float* q_row,
                              const float* lp_row, int B, int C, int ld, float grad_scale, float* row_loss, void* dl_planes,
                              size_t plane, int ld16, int rows16, float* d_a, float* s_row, void* stream);

/* column sums: out[n] = beta * out[n] + sum_m X[m,n]  (bias gradients; beta = 1 accumulates straight into
 * an existing .grad); two deterministic passes over row groups, `workspace` = renet_colsum_workspace(M, N)
 * bytes (0 for short matrices). */
size_t renet_colsum_workspace(int M, int N);
int renet_colsum(const float* X, int M, int N, int ldx, float* out, float beta, float* workspace,
                 size_t workspace_bytes, void* stream);

/* x[0..n) *= *scale, with the factor read from DEVICE memory (an upstream autograd gradient: no host sync);
 * a factor of exactly 1 returns without touching x. */
int renet_scale_by_device_scalar(float* x, size_t n, const float* scale, void* stream);
/* The same, additionally writing *bound_out = |*scale| * bound_in: the caller's bound on max |x| carried through the
 * scaling (operand bound of renet_gemm_f32_h3) without a pass over x. */
int renet_scale_by_device_scalar_bound(float* x, size_t n, const float* scale, float bound_in, float* bound_out,
                                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sequence assembly (Aggregator.py:142-165): builds the GRU inputs directly in PACKED time-major
 * layout (the .data of the PackedSequence the reference returns), with the dropout of
 * Aggregator.py:157-158 fused.  Row p of the packed layout belongs to sequence seq[p] (position in
 * the length-sorted batch):
 *   X [p,:] = drop([ h2[subj_row[p]] | ent[s[seq[p]]] | rel[r[seq[p]]] | glob[glob_row[p]] ])   (4D)
 *   Xr[p,:] = drop([ h2[subj_row[p]] | ent[s[seq[p]]] |                  glob[glob_row[p]] ])   (3D)
 * Masks are counter-based: keep(seed_x, p*4D+c), keep(seed_xr, p*3D+c).
 * Backward: dRows[p,:]  = grad wrt the gathered h2 row of packed row p (X and Xr parts);
 *           dEntSeq[i,:], dRelSeq[i,:] (i < B) = grad wrt ent[s_i] / rel[r_i] summed over the steps of
 *           sequence i (packed row of step j = step_off[j] + i; step_off is a DEVICE array [L+1]);
 *           rows of sequences without history come out zero.  The caller scatters the three with
 *           renet_segment_add.
 * ---------------------------------------------------------------------------------------------- */
int renet_seq_assemble_fwd(const float* h2, const float* ent, const float* rel, const float* glob,
                           const int32_t* subj_row, const int32_t* row_ent, const int32_t* row_rel,
                           const int32_t* glob_row, int S, int D, float drop_p, uint64_t seed_x,
                           uint64_t seed_xr, float* X, float* Xr, void* stream);
/* The same, additionally emitting the operand bounds of renet_gemm_f32_h3 for X and Xr: partX / partXr receive
 * renet_bound_parts(S * D) floats each (one maximum of |value written| per workgroup), so that no separate
 * renet_maxabs_partials pass over the 51 + 38 MB is needed.  S > 0. */
int renet_bound_parts(size_t total4);
int renet_seq_assemble_fwd_bounds(const float* h2, const float* ent, const float* rel, const float* glob,
                                  const int32_t* subj_row, const int32_t* row_ent, const int32_t* row_rel,
                                  const int32_t* glob_row, int S, int D, float drop_p, uint64_t seed_x,
                                  uint64_t seed_xr, float* X, float* Xr, float* partX, float* partXr, void* stream);
int renet_seq_assemble_bwd(const float* dX, const float* dXr, const int32_t* step_off, int L, int S,
                           int B, int D, float drop_p, uint64_t seed_x, uint64_t seed_xr, float* dRows,
                           float* dEntSeq, float* dRelSeq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GRU over the packed <= seq_len window (torch.nn.GRU semantics, 1 layer, h0 = 0, gate order r,z,n;
 * model.py:28-29,86,94; global_model.py:25,49).  Gi = X @ W_ih^T + b_ih is computed by the caller
 * with renet_gemm_f32; these entry points run the recurrence.
 *   Gi      [S, 3H]  packed time-major (step j occupies rows [off[j], off[j+1]), sequence i of the
 *                    length-sorted batch is row off[j]+i; batch_sizes non-increasing)
 *   step_off[L+1]    HOST array of row offsets (off[0] = 0, off[L] = S)
 *   Whh [3H,H], bhh[3H]
 *   h_last  [out_rows,H] state of every sequence after its own last step (h_n of nn.GRU), B = off[1];
 *                    rows [B, out_rows) are written as zeros (the reference pads h_n for the empty
 *                    histories, model.py:88): out_rows >= B
 *   saved   [S, 5H]  per packed row: r, z, n, (W_hn h + b_hn), h_prev   (consumed by backward)
 * Backward: given dh_last[B,H] produces dGi[S,3H], dGh[S,3H] (caller forms dW_ih, dW_hh, biases,
 * dX with renet_gemm_f32 / renet_colsum).
 * `workspace` = renet_gru_workspace(B, H) bytes per GRU (B = the largest first-step batch size of the
 * GRUs of the call), for both directions: the bf16 planes of W_hh (forward) / W_hh^T and its planes
 * (backward), then the state that travels between the per-step launches (bf16 planes of h / dGh, ping-pong,
 * and the fp32 dh) -- the recurrent products run as "bf16x6" like renet_gemm_f32_split unless RENET_GEMM=f32
 * selects the exact-fp32 MFMA kernels (one persistent launch, no per-step state: B may then be 0).
 * ---------------------------------------------------------------------------------------------- */
size_t renet_gru_workspace(int B, int H);
int renet_gru_fwd(const float* Gi, const int32_t* step_off, int L, int H, const float* Whh,
                  const float* bhh, float* h_last, int out_rows, float* saved, float* workspace,
                  size_t workspace_bytes, void* stream);
int renet_gru_bwd(const float* dh_last, const int32_t* step_off, int L, int H, const float* Whh,
                  const float* saved, float* dGi, float* dGh, float* workspace,
                  size_t workspace_bytes, void* stream);
/* n (1..4) independent GRUs over the SAME packed layout in one launch (RE-Net's `encoder` and
 * `encoder_r`, model.py:86,94): every pointer argument is a HOST array of n device pointers;
 * the workspace is n * renet_gru_workspace bytes. */
int renet_gru_fwd_multi(int n, const float* const* Gi, const int32_t* step_off, int L, int H,
                        const float* const* Whh, const float* const* bhh, float* const* h_last, int out_rows,
                        float* const* saved, float* workspace, size_t workspace_bytes, void* stream);
int renet_gru_bwd_multi(int n, const float* const* dh_last, const int32_t* step_off, int L, int H,
                        const float* const* Whh, const float* const* saved, float* const* dGi,
                        float* const* dGh, float* workspace, size_t workspace_bytes, void* stream);
/* n (<= 4) GRUs of up to TWO packed layouts in one launch: step_off[k] / L[k] / out_rows[k] describe problem k
 * (problems that pass the same step_off pointer share a layout).  The subject and the object pass of a training
 * step (train.py:136-137) are independent until their losses are added: their four recurrences -- ~60 workgroups
 * each -- then run side by side on the 256 CUs.  Equal Whh pointers are split into planes once. */
int renet_gru_fwd_layouts(int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H,
                          const float* const* Whh, const float* const* bhh, float* const* h_last,
                          const int* out_rows, float* const* saved, float* workspace, size_t workspace_bytes,
                          void* stream);
int renet_gru_bwd_layouts(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                          const float* const* Whh, const float* const* saved, float* const* dGi,
                          float* const* dGh, float* workspace, size_t workspace_bytes, void* stream);
/* The weight split of the two entries above as a call of its own, so that a caller can issue it early and on another
 * stream (the planes depend on nothing but W_hh).  renet_gru_split_weights issues exactly the split launches of
 * renet_gru_fwd_layouts (backward = 0: planes of W_hh) or renet_gru_bwd_layouts (backward != 0: planes of W_hh^T) for
 * the n weight pointers, into the same workspace slots (equal pointers are split once, into the slot of the first);
 * renet_gru_{fwd,bwd}_layouts_presplit are those entries without the split: they trust the slots.  The caller orders
 * the split before the recurrence and keeps the workspace untouched between them; forward and backward planes share
 * the slots.  RENET_ERR_UNSUPPORTED where the plain entries do not read planes from fixed slots (RENET_GEMM=f32,
 * RENET_GRU=steps): call the plain entries then. */
int renet_gru_split_weights(int n, const float* const* Whh, int H, int backward, float* workspace,
                            size_t workspace_bytes, void* stream);
int renet_gru_fwd_layouts_presplit(int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H,
                                   const float* const* Whh, const float* const* bhh, float* const* h_last,
                                   const int* out_rows, float* const* saved, float* workspace, size_t workspace_bytes,
                                   void* stream);
int renet_gru_bwd_layouts_presplit(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L,
                                   int H, const float* const* Whh, const float* const* saved, float* const* dGi,
                                   float* const* dGh, float* workspace, size_t workspace_bytes, void* stream);
/* renet_gru_bwd_layouts that additionally emits the operand bound of dGi for renet_gemm_f32_h3: bounds[k] receives
 * renet_gru_bound_parts(max over the problems of their sequence count) floats, one maximum of |dGi| per workgroup
 * (|dGh| <= |dGi| elementwise: the same bound serves both).  Only the persistent bf16x6 recurrence emits them;
 * RENET_ERR_UNSUPPORTED otherwise (RENET_GEMM=f32, RENET_GRU=steps) -- call the plain entry then. */
int renet_gru_bound_parts(int max_rows);
int renet_gru_bwd_layouts_bounds(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                                 const float* const* Whh, const float* const* saved, float* const* dGi,
                                 float* const* dGh, float* const* bounds, float* workspace, size_t workspace_bytes,
                                 void* stream);
/* The same recurrences with EXACT fp32 products (v_mfma_f32_16x16x4_f32) whatever RENET_GEMM says: the per-model form of the
 * exact mode (round 5; `net.gemm_mode = 'f32'`).  RENET_GEMM=f32 makes the plain entries above behave like these. */
int renet_gru_fwd_layouts_f32(int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H,
                              const float* const* Whh, const float* const* bhh, float* const* h_last,
                              const int* out_rows, float* const* saved, float* workspace, size_t workspace_bytes,
                              void* stream);
int renet_gru_bwd_layouts_f32(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                              const float* const* Whh, const float* const* saved, float* const* dGi,
                              float* const* dGh, float* workspace, size_t workspace_bytes, void* stream);
/* The same recurrences in bf16 mode (BASELINE config 5): W_hh and the hidden state / gate gradients are rounded to
 * bf16 (RNE) as MFMA operands -- ONE v_mfma_f32_16x16x32_bf16 product per fragment pair instead of the six of the
 * fp32-class split, a third of the W_hh stream -- with fp32 accumulation, fp32 gate math, fp32 state and outputs. */
int renet_gru_fwd_layouts_bf16(int n, const float* const* Gi, const int32_t* const* step_off, const int* L, int H,
                               const float* const* Whh, const float* const* bhh, float* const* h_last,
                               const int* out_rows, float* const* saved, float* workspace, size_t workspace_bytes,
                               void* stream);
int renet_gru_bwd_layouts_bf16(int n, const float* const* dh_last, const int32_t* const* step_off, const int* L, int H,
                               const float* const* Whh, const float* const* saved, float* const* dGi,
                               float* const* dGh, float* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Score head (model.py:89-91, 98-100).
 * renet_concat3_fwd/bwd : feat[b,:] = drop([ a[ia[b]] | hmid[b] | c[ic[b]] ])   (c may be NULL: 2 parts)
 * renet_softmax_ce      : per-row loss_b = logsumexp(logits[b,:]) - logits[b,target[b]];
 *                         loss_sum += sum_b loss_b (one float, zeroed by the caller);
 *                         if dlogits != NULL: dlogits = (softmax - onehot) * grad_scale  (may alias logits)
 * ---------------------------------------------------------------------------------------------- */
int renet_concat3_fwd(const float* a, const int32_t* ia, const float* hmid, const float* c,
                      const int32_t* ic, int B, int D, float drop_p, uint64_t seed, float* feat,
                      void* stream);
/* The same with the operand bound of feat: bound_part receives renet_bound_parts(B * parts * D / 4) floats. */
int renet_concat3_fwd_bounds(const float* a, const int32_t* ia, const float* hmid, const float* c,
                             const int32_t* ic, int B, int D, float drop_p, uint64_t seed, float* feat,
                             float* bound_part, void* stream);
int renet_concat3_bwd(const float* dfeat, int B, int D, int parts, float drop_p, uint64_t seed,
                      float* da_rows, float* dhmid, float* dc_rows, void* stream);
/* y = x * keepmask(seed) / (1 - p) on float4 groups (n % 4 == 0); its own backward (apply to dy).
 * Used for the dropout of Aggregator.py:69 (global model sequence tensor). */
int renet_dropout(const float* x, size_t n, float drop_p, uint64_t seed, float* y, void* stream);
int renet_softmax_ce(const float* logits, const int32_t* target, int B, int C, int ld,
                     float grad_scale, float* row_loss, float* dlogits, void* stream);
/* renet_softmax_ce for the loss THROUGH THE COPY MIX of the recurrence prior (renet_recurrence_mix_rows): per row b the gate
 * a_row[b] in [0, 1) and the prior's mass on the gold column q_row[b] = w[target] / W (renet_recurrence_gold_rows), device
 * fp32 [B].  The caller has zeroed a_row where the prior abstains; the kernel trusts it.  With p = softmax(logits[b, :]),
 * g = target[b]:
 *     m = (1 - a) p_g + a q,   row_loss[b] = -log m,   s_b = (1 - a) p_g / m  in [0, 1]
 *     dlogits[b, c] = (p_c - [c == g]) * (grad_scale * s_b)          (NULL: not written; may alias logits)
 *     d_a[b]        = grad_scale * (p_g - q) / m                     (NULL: not written)
 * Where a == 0 or q == 0: s_b = 1 exactly -- the gradient row of renet_softmax_ce bit for bit -- row_loss = (logsumexp - x_g)
 * - log1p(-a), and p_g, which may underflow to 0, is not divided by: d_a = grad_scale * (p_g - q) / ((1 - a) p_g), 0 where
 * p_g == 0.  The same kernels as renet_softmax_ce (their MIX instances, chosen by the same widths), fp32 arithmetic; the
 * per-row scalars cost no pass over the row.  A missing array or ld < C: RENET_ERR_BADARG before any launch. */
int renet_mix_ce(const float* logits, const int32_t* target, const float* a_row, const float* q_row, int B, int C, int ld,
                 float grad_scale, float* row_loss, float* dlogits, float* d_a, void* stream);
/* renet_mix_ce for the loss THROUGH THE JOINT MIX of renet_joint_mix_rows: the entity head's writer of an EVENT loss.  Beside
 * a_row and q_row (renet_joint_gold_rows: q = G / W, entity-wide W), lp_row[b] <= 0 (device fp32 [B]) is the log-probability
 * the relation head gives ITS gold class, pr = exp(lp).  With p = softmax(logits[b, :]), g = target[b]:
 *     m = (1 - a) p_g pr + a q,   row_loss[b] = -log m   (= -M[r*, g] of renet_joint_mix_rows),   s_b = (1 - a) p_g pr / m
 *     dlogits[b, c] = (p_c - [c == g]) * (grad_scale * s_b)          (NULL: not written; may alias logits)
 *     d_a[b]        = grad_scale * (p_g pr - q) / m                  (NULL: not written)
 *     s_row[b]      = s_b                                            (NULL: not written)
 * The relation head's gradient row is ITS plain CE gradient times the same s_b (the caller scales it), and dL/dq = -a exp(L).
 * p_g pr = exp(x_g + lp - max) / sum: the kernels of renet_mix_ce with the gold logit x_g + lp_row[b] (one fp32 addition), so
 * lp_row = 0 gives renet_mix_ce bit for bit, and its branches hold with p_g pr in p_g's place: where a == 0 or q == 0, s_b = 1
 * exactly, row_loss = (logsumexp - x_g - lp) - log1p(-a), and a product that underflowed to 0 is not divided by (d_a = 0).
 * Refusals as renet_mix_ce, and a missing lp_row. */
int renet_joint_mix_ce(const float* logits, const int32_t* target, const float* a_row, const float* q_row, const float* lp_row,
                       int B, int C, int ld, float grad_scale, float* row_loss, float* dlogits, float* d_a, float* s_row,
                       void* stream);
/* Softmax cross-entropy against SPARSE SOFT targets (the global model's loss, global_model.py:52-55, with the target
 * distribution of row b given as the entries k in [tgt_ptr[b], tgt_ptr[b + 1]): columns tgt_col[k] -- distinct, ascending,
 * in [0, C) -- with weights tgt_w[k] >= 0 that need NOT sum to 1).  With W = sum_k tgt_w[k] and p = softmax(logits[b, :]):
 *   row_loss[b]   = W * logsumexp(logits[b, :]) - sum_k tgt_w[k] * logits[b, tgt_col[k]]
 *   dlogits[b, c] = grad_scale * (W * p_c - w_c)          (w_c = the weight of column c, 0 if it is not a target)
 * dlogits may be NULL (loss only) or alias logits (in place).  An empty row gives loss 0 and a zero gradient; a -inf logit
 * gives gradient 0 in its column.  ld >= C is the row stride (elements) of logits and dlogits; nothing outside the
 * [B, C] block is touched.  No atomics: the result is a function of the inputs alone.  (csrc/soft_ce.hip) */
int renet_soft_ce_sparse(const float* logits, int B, int C, int ld, const int32_t* tgt_ptr, const int32_t* tgt_col,
                         const float* tgt_w, float grad_scale, float* row_loss, float* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-graph readout of the global model (Aggregator.py:58-61 dgl.max_nodes / mean_nodes):
 *   out[g,:] = max / mean over rows [seg_ptr[g], seg_ptr[g+1]) of h; argmax[g,:] saved for backward. */
int renet_segment_pool_fwd(const float* h, const int32_t* seg_ptr, int G, int D, int is_max,
                           float* out, int32_t* argmax, void* stream);
int renet_segment_pool_bwd(const float* dout, const int32_t* seg_ptr, const int32_t* argmax, int G,
                           int D, int is_max, int N, float* dh, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbour pooling of the mean / attentive history encoders (Aggregator.py:239-361: MeanAggregator, AttnAggregator;
 * replaces the sparse.mm + division of :264-267, the per-sequence loops of :276-278 / :322-340 and
 * pack_padded_sequence).  A SEGMENT is the neighbour list of one time step of one sequence:
 *   nbr[seg_ptr[u] .. seg_ptr[u + 1])  entity ids (rows of E [N_ent, D]); repeats allowed, never empty
 *   seg_s[u], seg_r[u]                 the sequence's subject entity / relation (row of R [N_rel, D])
 *   seg_q[u]                           the sequence's row in q
 *   out_row[u]                         the segment's row in the packed (time-major) output
 * attn == 0:  out[out_row[u]] = [ mean_j E[nbr_j] | E[s] ]                                    (row stride 2D)
 * attn != 0:  a_j = v . tanh(P[nbr_j] + q[seg_q[u]]),  w = softmax_j(a)                         (Aggregator.py:333-337)
 *             out[out_row[u]] = [ sum_j w_j E[nbr_j] | E[s] | R[r] ]                          (row stride 3D)
 *             with P [N_ent, D] = E W_o^T and q = W_s E[s] + W_r R[r] + b computed by the caller (renet_gemm_*);
 *             stats[u] = (max_j a_j, log sum_j exp(a_j - max)), w[k] = the softmax weight of neighbour k.
 * seg_ptr is read on the device; seg_ptr_host is the same array in HOST memory, checked here: a segment of length 0
 * returns RENET_ERR_BADARG.  One wave per segment, an online softmax (running maximum, rescaled only when it moves);
 * segments longer than 256 neighbours are split over the waves of a workgroup and merged in wave order.  No atomics:
 * the result is a function of the inputs alone.
 * Backward (dOut: the gradient of the packed rows, out: the forward result), per neighbour k of segment u, with
 * g = dOut[out_row[u], 0:D]:
 *   attn == 0:  cE[k] = g / n_u
 *   attn != 0:  da = w_k (g . E[nbr_k] - g . out[out_row[u], 0:D]),  t = tanh(P[nbr_k] + q)
 *               cE[k] = w_k g,  cP[k] = da v (1 - t^2),  dq_rows[u] = sum_k cP[k],  dv_rows[u] = sum_k da t
 *   ds_rows[u] / dr_rows[u] = the E[s] / R[r] column blocks of dOut[out_row[u]] (dr_rows: attn only).
 * The caller sums cE / cP per destination entity (renet_segment_add2 over a plan of nbr), dq_rows / ds_rows / dr_rows
 * per sequence (renet_segment_add) and dv_rows over all segments (renet_colsum); arguments a mode does not use may be
 * NULL.  fp32 only; every float pointer 16-byte aligned. */
int renet_nbr_pool_fwd(const float* E, const float* R, const float* P, const float* q, const float* v,
                       const int32_t* nbr, const int32_t* seg_ptr, const int32_t* seg_ptr_host, const int32_t* seg_s,
                       const int32_t* seg_r, const int32_t* seg_q, const int32_t* out_row, int S, int D, int attn,
                       float* out, float* stats, float* w, void* stream);
int renet_nbr_pool_bwd(const float* dOut, const float* out, const float* E, const float* P, const float* q,
                       const float* v, const float* w, const int32_t* nbr, const int32_t* seg_ptr,
                       const int32_t* seg_ptr_host, const int32_t* seg_q, const int32_t* out_row, int S, int D, int attn,
                       float* cE, float* cP, float* dq_rows, float* dv_rows, float* ds_rows, float* dr_rows,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused clip_grad_norm_ + Adam (+ weight decay) + zero_grad over flat buffers (train.py:140-142).
 * p, g, m, v: n floats each (16-byte aligned); `step` is the 1-based step count (bias correction);
 * max_norm <= 0 disables clipping; grad_norm_out (optional device float) receives the pre-clip norm.
 * torch.optim.Adam semantics (L2 weight decay added to the clipped gradient). */
size_t renet_adam_workspace(size_t n);
int renet_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float max_norm, int step, int zero_grad, float* workspace,
                    size_t workspace_bytes, float* grad_norm_out, void* stream);
/* The same step on the gradient g * grad_scale (norm, clip coefficient and update all see the scaled gradient):
 * grad_scale = 1 / world_size turns the SUM all-reduce of the data-parallel exchange into the mean without a
 * separate pass over the 81 MB buffer (the reference has no distributed step; train.py:140-142 on the averaged
 * gradient is what gradient accumulation over world_size batches would do). */
int renet_adam_step_scaled(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, float max_norm, float grad_scale, int step,
                           int zero_grad, float* workspace, size_t workspace_bytes, float* grad_norm_out,
                           void* stream);

/* The same step with the sum of squares ALREADY accumulated per region of the flat gradient (data-parallel runs: each
 * all-reduce bucket's partials are computed on the reducer's stream as the bucket arrives, so that only this scalar combine
 * is left of clip_grad_norm_, train.py:140, when the last bucket lands):
 *   renet_sumsq_partials      : partial[0..n_slots) = per-workgroup sums of g[i]^2 over g[0..n) (fixed order: deterministic;
 *                               slots without elements receive 0); g 16-byte aligned; n_slots <= 2048
 *   renet_adam_step_presummed : renet_adam_step_scaled without its own norm pass: ||g||^2 = sum of partial[0..n_partial) */
int renet_sumsq_partials(const float* g, size_t n, float* partial, int n_slots, void* stream);
int renet_adam_step_presummed(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, float max_norm, float grad_scale, int step, int zero_grad,
                              const float* partial, int n_partial, float* grad_norm_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference: the joint (relation, object) distribution of pred_r_rank2 and its top-k (model.py:205-209,239).
 *   renet_joint_softmax : logits [n * R, N] (row stride ld) is overwritten, row (e, r) with
 *                           softmax(logits[e, r, :]) * softmax(logits_r[e, :])[r] * prob_e[e]
 *                         (the reference: torch.softmax x2 + two broadcast multiplies); any N, R <= 1024 (beyond that
 *                         RENET_ERR_UNSUPPORTED).  N * 4 <= 128 KB: one read and one write, the row staged in LDS; wider
 *                         rows are streamed twice (an online max / sum sweep, then the write: the same operation order
 *                         per element, the row sum rounded in another order).
 *   renet_topk_positive : the k largest elements of every row of x [n, M] (row stride ldx), x >= 0: values and int64
 *                         column indices, in NO particular order (torch.topk(..., sorted=False)); exact (radix select
 *                         on the bit pattern); ties at the threshold are broken arbitrarily.
 *                         workspace: renet_topk_workspace(n) bytes. */
int renet_joint_softmax(float* logits, int ld, int n, int R, int N, const float* logits_r, int ld_r,
                        const float* prob_e, void* stream);
size_t renet_topk_workspace(int n);
int renet_topk_positive(const float* x, size_t ldx, int n, int M, int k, float* out_val, int64_t* out_idx,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference: the evaluation metric (model.py:365-381 raw, 391-418 filtered; the loss of 358-361).  One read of every row of
 * scores [n, C] (row stride ld; never written) gives, for the gold column label[i] of row i,
 *   greater[i]  = number of columns whose value is  > the gold value,
 *   equal[i]    = number of columns whose value is == the gold value, the gold column included
 *                 (the reference's rank with averaged ties is greater + (equal - 1) / 2 + 1),
 *   row_loss[i] = logsumexp(scores[i, :]) - scores[i, label[i]]   (renet_softmax_ce without a gradient; NULL: not computed).
 * filtered = 0: the values are the scores themselves; filt_ptr must be NULL.
 * filtered = 1: the values are sigmoid(score) as torch.sigmoid rounds it in fp32 (1 / (1 + exp(-x)): distinct logits that
 *   collapse onto one sigmoid value, 1.0 or 0 included, tie exactly as in the reference), and every column listed in
 *   filt_col[filt_ptr[i] .. filt_ptr[i + 1]) other than label[i] counts with the value 0 instead of its own (filt_ptr NULL:
 *   no lists).  A column may be listed at most once per row; listed columns outside [0, C) are ignored.
 * label[i] is device data, so it cannot be checked here: a label outside [0, C) is clamped into the row by the kernel.
 * RENET_ERR_BADARG for n < 0, C < 1, ld < C, a missing array, or lists with filtered = 0; n == 0 is a no-op. */
int renet_rank_rows(const float* scores, int ld, int n, int C, const int32_t* label, const int32_t* filt_ptr,
                    const int32_t* filt_col, int filtered, int32_t* greater, int32_t* equal, float* row_loss,
                    void* stream);

/* The three metric settings of one score matrix from ONE read of every row: counts [6, n] (int32, row-major) =
 *   raw greater, raw equal            -- renet_rank_rows(filtered = 0),
 *   filtered greater, equal           -- renet_rank_rows(filtered = 1) with the list `a` (time-agnostic: the other completions
 *                                        known at ANY time),
 *   time_filtered greater, equal      -- the same rule with the list `t` (time-aware: the other completions known at the
 *                                        query's own timestamp; not in the reference),
 * and row_loss as above (NULL: not computed).  A list is addressed in place in a resident column table of len_x entries:
 * row i takes cols_x[start_x[i] .. start_x[i] + count_x[i]) (cut to the table; count <= 0: empty), every column at most once
 * per row, columns outside [0, C) ignored.  All three pointers of a list NULL: no list -- that setting then gives the
 * unfiltered sigmoid counts.  Both filtered settings are corrections of the same swept sigmoid counts, so they differ only in
 * their lists.  RENET_ERR_BADARG for n < 0, C < 1, ld < C, a missing array, a list with only some of its three pointers or
 * a negative length; n == 0 is a no-op. */
int renet_rank_rows3(const float* scores, int ld, int n, int C, const int32_t* label, const int32_t* cols_a,
                     const int32_t* start_a, const int32_t* count_a, int len_a, const int32_t* cols_t,
                     const int32_t* start_t, const int32_t* count_t, int len_t, int32_t* counts, float* row_loss,
                     void* stream);

/* Ranked, filtered top-k predictions (not in the reference): ONE read of every row of scores [n, C] (row stride ld; never
 * written) gives the k best CANDIDATES of row i: all columns minus those listed in cols[start[i] .. start[i] + count[i])
 * (a range of a resident column table of len entries, cut to the table; count <= 0: empty; every column at most once per row;
 * listed columns outside [0, C) ignored -- the list form of renet_rank_rows3), except that a listed column equal to keep[i]
 * stays a candidate (keep NULL, or an entry outside [0, C): nothing is exempt).  All three list pointers NULL: no list.
 *   out_idx [n, k], out_val [n, k] : the candidates by score descending, then column ascending (float comparison: -0.0 and
 *                                    +0.0 tie; ties at the k-th value go to the lower columns: the result is deterministic);
 *                                    out_val holds the scores themselves, bit for bit (a -0.0 as +0.0).
 *   out_n [n]                      : min(k, number of candidates); the slots from out_n[i] on hold index -1, value -inf,
 *                                    logp -inf.
 *   out_logp [n, k]                : out_val - logsumexp(scores[i, 0 .. C)) over ALL columns, listed ones included (the
 *                                    model's own log-probability: the filter removes candidates, not mass), the logsumexp
 *                                    online in fp64 as for row_loss above, one rounding; NULL: not computed.
 * Scores are finite or -inf: a -inf score is an ordinary candidate that sorts last (logp -inf), distinct from a filtered
 * column.  A NaN (ranked below -inf) or +inf gives no meaningful order or logp, but never an index outside [-1, C).
 * 1 <= k <= 1024 (k may exceed C); C <= 32768 (the row is staged in LDS), beyond that RENET_ERR_UNSUPPORTED, before any
 * launch (wider rows: renet_topk_rows_wide below).  RENET_ERR_BADARG for n < 0, C < 1, ld < C, k out of range, a negative len, a list with only some of its three
 * pointers or a missing output array; n == 0 is a no-op. */
int renet_topk_rows(const float* scores, int ld, int n, int C, int k, const int32_t* cols, const int32_t* start,
                    const int32_t* count, int len, const int32_t* keep, int32_t* out_idx, float* out_val, float* out_logp,
                    int32_t* out_n, void* stream);

/* The same contract, result for result, for rows beyond one CU's LDS: any C up to RENET_TOPK_ROWS_WIDE_MAX_C, beyond that
 * RENET_ERR_UNSUPPORTED, before any launch (narrower rows are served too).  The row is taken in pieces of stage_cols columns
 * (0: the entry's own choice, an even split into pieces of at most 15360 columns; else 64 <= stage_cols <= 32768, anything
 * else RENET_ERR_BADARG): a (piece, row) grid leaves every piece's sorted min(k, stage_cols) best candidates, its candidate
 * count and its fp64 (max, sum of exponentials) in the workspace, and one workgroup per row merges the pieces in column
 * order.  A list is applied by every piece it reaches, each listed column by the one piece that holds it; out_n comes from
 * the sum of the pieces' counts; the logsumexp is the fixed-order fp64 combination of the pieces' pairs (one rounding of
 * out_logp, as above).  No global atomics: the result is the same from run to run, and scores is never written.
 * workspace: renet_topk_rows_wide_workspace bytes for the same n, C, k, stage_cols (0 for arguments the entry refuses),
 * 8-byte aligned; too small, misaligned or NULL: RENET_ERR_WORKSPACE.  The other refusals are those of renet_topk_rows. */
#define RENET_TOPK_ROWS_WIDE_MAX_C (1 << 20)
size_t renet_topk_rows_wide_workspace(int n, int C, int k, int stage_cols);
int renet_topk_rows_wide(const float* scores, int ld, int n, int C, int k, const int32_t* cols, const int32_t* start,
                         const int32_t* count, int len, const int32_t* keep, int32_t* out_idx, float* out_val,
                         float* out_logp, int32_t* out_n, int stage_cols, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Joint (relation, entity) ranks of an event (not in the reference; csrc/joint_rank.hip).  scores [G * R, C] (row stride ld;
 * never written) holds, for each of G histories ("groups"), the R logits rows of the entity head -- row g * R + r the query
 * whose relation is r -- and logits_r [G, R] (row stride ld_r) the relation head's rows.  The joint log-probability of the
 * pair (r, c) of group g is
 *   J[g, r, c] = scores[g * R + r, c] + off[g * R + r]                      (ONE IEEE fp32 addition, never contracted)
 *   off[g * R + r] = fp32( logsoftmax(logits_r[g, :])[r] - logsumexp(scores[g * R + r, 0 .. C)) ),
 * both terms in fp64 from the fp32 inputs (the online logsumexp of row_loss above), rounded once.
 * renet_joint_row_offsets writes off [G * R] from one read of the block; any C, any row alignment, 1 <= R <= 1024.
 * RENET_ERR_BADARG for G < 0, R out of range, C < 1, ld < C, ld_r < R or a missing array; G == 0 is a no-op. */
int renet_joint_row_offsets(const float* scores, int ld, int G, int R, int C, const float* logits_r, int ld_r,
                            float* off_out, void* stream);

/* Query q (of Q) ranks its gold pair (gold_r[q], gold_c[q]) among the R * C pairs of group[q], on the fp32 values J above
 * with the gold value v = J[group[q], gold_r[q], gold_c[q]]: one workgroup per (q, r) sweeps row group[q] * R + r once.  Per
 * row q * R + r (all outputs row-major):
 *   counts [6, Q * R]  : raw greater (#c: J > v), raw equal (#c: J == v, the gold pair included), then the same two of the
 *                        filtered and of the time_filtered setting.  The settings' lists are per (q, r) row, addressed in
 *                        place in a resident column table as in renet_rank_rows3: row q * R + r takes
 *                        cols_x[start_x[q * R + r] .. + count_x[q * R + r]) (cut to the table; count <= 0: empty; every
 *                        column at most once per row; columns outside [0, C) ignored).  A listed column is NO candidate --
 *                        it loses its contribution (the renet_topk_rows convention) -- except the gold pair itself, which
 *                        always stays.  All three pointers of a list NULL: no list, the raw counts.
 *   at_gold [Q * R]    : J[group[q], r, gold_c[q]] (the R values among which a relation is ranked given both endpoints)
 *   listed [2, Q * R]  : 1 where gold_c[q] is on the row's list a / list t, else 0.
 * The sum of a query's R rows of counts gives its pair rank: greater + (equal - 1) / 2 + 1.  group, gold_r and gold_c are
 * device data: values outside [0, G), [0, R), [0, C) are clamped into range by the kernel.  No global atomics.
 * RENET_ERR_BADARG for Q < 0, G < 1, R < 1, C < 1, ld < C, a missing array, a list with only some of its three pointers or
 * a negative length; Q == 0 is a no-op. */
int renet_joint_rank_rows(const float* scores, int ld, int G, int C, int R, const float* off, int Q, const int32_t* group,
                          const int32_t* gold_r, const int32_t* gold_c, const int32_t* cols_a, const int32_t* start_a,
                          const int32_t* count_a, int len_a, const int32_t* cols_t, const int32_t* start_t,
                          const int32_t* count_t, int len_t, int32_t* counts, float* at_gold, int32_t* listed,
                          void* stream);

/* Global choice of the generated events of a timestamp (reference model.py:229-258: the num_k best continuations over all
 * sampled entities, an entity sampled m times counted m times; csrc/event_select.hip; the host statement is
 * tests/event_select_statement.py).  One call takes the per-row top-k lists of one joint block of G entities ("groups") x
 * R relation rows -- ent / val [G * R, k]: renet_topk_rows' out_idx / out_val (a row sorted by value descending, empty slots
 * -1 / -inf), off [G * R]: renet_joint_row_offsets, g_ent / g_lprior / g_mult [G]: the group's entity id, log prior and
 * multiplicity (>= 1; a smaller value counts as 1) -- and the winners carried from the blocks before it (in_*: [num_k]
 * each, in_n[1] on the device, the layout of the outputs; all six NULL: none).
 *   Candidates : slot j of row g * R + r with ent >= 0: value V = (val + off[g * R + r]) + g_lprior[g] (two IEEE fp32
 *                additions in that order, never contracted), identity (g_ent[g], r, ent), weight g_mult[g]; a -inf value
 *                is an ordinary candidate that sorts last.  The first min(in_n, num_k) carry entries are candidates too,
 *                with the values and weights they carry.
 *   Order      : V descending (float comparison: -0.0 and +0.0 tie), then carry entries in their stored order before block
 *                candidates, then flat position (g * R + r) * k + j ascending.  With the groups in ascending entity order,
 *                every entity in one block only, and renet_topk_rows' ties towards the lower column, that is (given
 *                entity, relation, other entity) ascending: the result is a deterministic function of the inputs.
 *   Output     : the shortest prefix of that order whose summed weight reaches num_k (all candidates if the total is
 *                smaller), in that order: out_given / out_rel / out_other / out_val / out_mult [num_k], out_n[1] its length
 *                (<= num_k, as weights are >= 1); the slots behind out_n hold -1, -1, -1, -inf, 0.  Selection composes:
 *                the prefix over several blocks is the fold of this call over the blocks, each call's outputs the next
 *                one's carry.  G == 0 selects among the carry alone: a carry this entry wrote comes back as it is.
 * Only the first min(k, num_k) slots of a row are read (a row is sorted).  A NaN value sorts below -inf.  1 <= R, k, num_k
 * <= 1024.  A weighted radix select over a 64-bit (value, place) key that is unique per candidate, then one workgroup
 * sorts the at most num_k winners: no host synchronisation, integer atomics only, the same result from run to run.
 * Outputs must not alias inputs.  workspace: renet_select_events_workspace bytes (0 for arguments the entry refuses),
 * 8-byte aligned; too small, misaligned or NULL: RENET_ERR_WORKSPACE.  RENET_ERR_BADARG for G < 0, R, k or num_k out of
 * range, a missing array, or a carry with only some of its six pointers; G * R * k beyond int32: RENET_ERR_UNSUPPORTED;
 * every refusal comes before any launch. */
size_t renet_select_events_workspace(int G, int R, int k, int num_k);
int renet_select_events(const int32_t* ent, const float* val, const float* off, const int32_t* g_ent, const float* g_lprior,
                        const int32_t* g_mult, int G, int R, int k, int num_k, const int32_t* in_given,
                        const int32_t* in_rel, const int32_t* in_other, const float* in_val, const int32_t* in_mult,
                        const int32_t* in_n, int32_t* out_given, int32_t* out_rel, int32_t* out_other, float* out_val,
                        int32_t* out_mult, int32_t* out_n, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE batch-graph builder for the merged training batch (both directions of train.py:136-137 as one batch of 2B
 * sequences: graph.build_batch_both; replaces utils.py:209-244 + 115-131 + dgl.batch and this library's own HOST
 * builder for that case).  The dataset is resident in HBM (RenetStoreDev: quadruples, the per-role history index of
 * preprocess.HistoryIndex, the per-timestamp fact lists of graph.GraphStore); one call takes the B quadruple indices of
 * a batch (device int32) and fills the caller's output arrays with EXACTLY the arrays the host builder produces
 * (graph.HostBatch; tests/test_gpu_builder.py compares them bit for bit).  No host synchronisation inside: every stage
 * launches over the capacities and guards on the device-side counts, which the caller copies back (RENET_BB_NCOUNTS
 * int32) when it needs the sizes.  counts[RENET_BB_ERR] != 0 => a capacity was exceeded (or a timestamp was not in the
 * store): the outputs are invalid, rebuild with larger capacities / on the host. */
typedef struct {
    const int32_t *q_s, *q_r, *q_o;            /* [n_quads] the stream's quadruples */
    const int32_t* h_first[2];                 /* role 0 = subject histories, 1 = object histories: per quadruple the */
    const int32_t* h_count[2];                 /*   first snapshot of its window and the number of snapshots in it    */
    const int32_t* snap_t[2];                  /* [n_snap] timestamp of every snapshot                                */
    const int32_t* snap_ptr[2];                /* [n_snap + 1] neighbour range of every snapshot                      */
    const int32_t* nbr_o[2];                   /* [n_quads] neighbour entities                                        */
    const int32_t* times;                      /* [T] sorted timestamps of graph_dict                                 */
    const int32_t* trip_ptr;                   /* [T + 1] fact range of every timestamp                               */
    const int32_t *trip_s, *trip_r, *trip_o;   /* [n_facts]                                                           */
    const int32_t* glob_times;                 /* [n_glob] sorted timestamps of the global-embedding table            */
    int T, n_glob, n_facts, num_ent, num_rels;
} RenetStoreDev;

typedef struct {
    int32_t *node_ent, *node_slot, *row_ptr, *col, *etype;
    float* norm;
    int32_t *heavy_rows, *e_src, *e_dst, *chunk_ptr, *chunk_type, *type_chunk_ptr;
    int32_t *e_src2, *e_dst2, *chunk_ptr2, *chunk_type2, *type_chunk_ptr2;
    int32_t *it_src, *it_type, *grp_ptr;
    int32_t *subj_row, *row_seq, *row_ent, *row_rel, *glob_row;
    int32_t *s_sorted, *r_sorted, *rel_label, *ent_label, *perm, *step_off;
    int32_t* plan_order[4];                    /* 0: node_ent, 1: subj_row, 2: s_sorted, 3: r_sorted */
    int32_t* plan_seg[4];
    int32_t* plan_target[4];
    int32_t* counts;                           /* [RENET_BB_NCOUNTS] */
    int cap_nodes, cap_edges;
    int32_t* seg_ptr;                          /* [G + 1] node offsets of the member graphs: renet_build_full_graphs only */
} RenetBatchOut;

enum {
    RENET_BB_NNZ = 0, RENET_BB_S, RENET_BB_L, RENET_BB_TB, RENET_BB_FACTS, RENET_BB_N, RENET_BB_NA, RENET_BB_E2,
    RENET_BB_E, RENET_BB_NHEAVY, RENET_BB_NHEAVY_OUT, RENET_BB_NCHUNKS, RENET_BB_NCHUNKS2, RENET_BB_NITEMS,
    RENET_BB_NGROUPS, RENET_BB_NGROUPS_OUT, RENET_BB_NSEG0, RENET_BB_NSEG1, RENET_BB_NSEG2, RENET_BB_NSEG3,
    RENET_BB_ERR, RENET_BB_EOUT,             /* E_out = edges into the row prefix [0, nA) */
    RENET_BB_STEP_OFF = 24,                  /* counts[24 .. 56]: copy of step_off[0 .. 32] (the GRU launches need it on the host) */
    RENET_BB_NCOUNTS = 64
};
enum { RENET_BB_ERR_TIME = 1, RENET_BB_ERR_GLOB = 2, RENET_BB_ERR_NODES = 4, RENET_BB_ERR_EDGES = 8 };

size_t renet_build_batch_workspace(const RenetStoreDev* store, int B, int cap_nodes, int cap_edges);
int renet_build_batch_both(const RenetStoreDev* store, const int32_t* idx_dev, int B, int seq_len, int heavy_thresh,
                           int group_budget, int chunk, const RenetBatchOut* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HISTORY WINDOWS of arbitrary (entity, as_of) queries against the resident history index (csrc/builder_query.hip; the
 * host statement is preprocess.HistoryIndex.lookup, element for element).  ent_ptr0 / ent_ptr1 [num_ent + 1]: the snapshot
 * range of every entity in role 0 (subject histories) / 1 (object histories), snap_t0 / snap_t1 the snapshot timestamps of
 * RenetStoreDev.  ent[2][n]: per query its subject (row 0) and its object (row 1); as_of[n].  For pair (role, i), with sid
 * the first snapshot of the entity's range whose timestamp is >= as_of[i] (binary search):
 *     h_first[role][i] = max(range start, sid - history_len),  h_count[role][i] = sid - h_first[role][i]
 * and (0, 0) for an entity outside [0, num_ent): an absent side.  h_first / h_count [2][n] are what RenetStoreDev takes for
 * a store whose quadruples are the queries.  ONE launch over the 2 n pairs, no workspace, no synchronisation.  It exists so
 * that queries which already are device tensors become a builder batch without a host round trip. */
int renet_query_histories(const int32_t* ent_ptr0, const int32_t* ent_ptr1, const int32_t* snap_t0, const int32_t* snap_t1,
                          int num_ent, int history_len, const int32_t* ent, const int32_t* as_of, int n, int32_t* h_first,
                          int32_t* h_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * APPEND of newly observed facts to the resident history index of ONE role (csrc/builder_append.hip; the host statement
 * is preprocess.HistoryIndex.appended, array for array, and the result equals the HistoryIndex of the longer stream bit for
 * bit).  Old index (device int32, only read): ent_ptr [num_ent + 1], snap_t [n_snaps], snap_ptr [n_snaps + 1], nbr_o /
 * h_first / h_count [n_quads], and q_ent [n_quads], the entity of every old quadruple in this role (q_s for role 0, q_o for
 * role 1).  New facts (device int32 [m]), every timestamp >= every old one, SORTED stably by (entity, time, input order):
 * new_ent, new_t, new_other (the neighbour) and new_pos, the input position of each sorted fact -- new quadruple new_pos[j]
 * becomes position n_quads + new_pos[j] of the longer stream.  A new (entity, time) group whose time equals the entity's
 * last old snapshot joins that snapshot; every other group opens one.  Outputs (the caller's fresh allocations):
 * ent_ptr_out [num_ent + 1], snap_t_out [cap_snaps], snap_ptr_out [cap_snaps + 1], nbr_o_out / h_first_out / h_count_out
 * [n_quads + m]; totals[2] = (snapshots of the longer index, of which opened).  cap_snaps in [n_snaps, n_snaps + m] is what
 * the snapshot outputs hold: no store goes past it, and the outputs are complete when totals[0] == cap_snaps (a caller
 * that knows which entities were active at the last old timestamp knows the count beforehand).  m == 0 gives copies.  Runs
 * on `stream`, no host synchronisation, no atomics.  Negative sizes, a missing array, a capacity outside its range or a
 * workspace below renet_store_append_workspace(num_ent, m): RENET_ERR_BADARG; n_quads + m, n_snaps + m or num_ent + 1 beyond
 * int32: RENET_ERR_UNSUPPORTED, before any launch.
 * renet_append_i32: out[0 .. n_old + n_add) = old[0 .. n_old) followed by add[0 .. n_add) -- the flat arrays of the store
 * (quadruples, timestamps, fact lists), which an append only lengthens. */
size_t renet_store_append_workspace(int num_ent, int m);
int renet_store_append(const int32_t* ent_ptr, const int32_t* snap_t, const int32_t* snap_ptr, const int32_t* nbr_o,
                       const int32_t* h_first, const int32_t* h_count, const int32_t* q_ent, int num_ent, int n_snaps,
                       int n_quads, int history_len, const int32_t* new_ent, const int32_t* new_t, const int32_t* new_other,
                       const int32_t* new_pos, int m, int cap_snaps, int32_t* ent_ptr_out, int32_t* snap_t_out,
                       int32_t* snap_ptr_out, int32_t* nbr_o_out, int32_t* h_first_out, int32_t* h_count_out, int32_t* totals,
                       void* workspace, size_t workspace_bytes, void* stream);
int renet_append_i32(const int32_t* old, int n_old, const int32_t* add, int n_add, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RECURRENCE PRIOR on the resident stream (csrc/recurrence.hip): "what did (entity, relation) connect to before, how often,
 * how recently", as a non-learned baseline and as a copy term mixed into the model's scores.
 *
 * PAIR TABLES of one role (device int32 [n_facts] each): p_rel, p_other (the partner: o for role 0, s for role 1) and p_t
 * over ALL facts, sorted by (entity, relation, partner, time).  The facts of entity e are the index range
 * [snap_ptr[ent_ptr[e]], snap_ptr[ent_ptr[e + 1]]) of that role's history index (RenetStoreDev / renet_store_append): the
 * same range as there, another order inside it.  Duplicate facts stay.  Host statement: preprocess.PairIndex.
 *
 * renet_pair_append: the tables after m new facts were appended, WITHOUT a sort of the old ones (host statement:
 * preprocess.PairIndex.appended, array for array; the result equals the tables of the longer stream bit for bit).  Inputs:
 * the old tables [n]; ent_ptr / snap_ptr of the old index and ent_ptr_new / snap_ptr_new of the longer one (outputs of
 * renet_store_append) with their snapshot counts; the new facts new_ent / new_rel / new_other / new_t [m], sorted by
 * (entity, relation, partner, time).  Outputs: the caller's fresh p_rel_out / p_other_out / p_t_out [n + m].  One thread per
 * old and per new fact, a binary search each inside one entity's range; no atomics, no read-back, no workspace; the old
 * tables are only read.  Negative sizes or a missing array: RENET_ERR_BADARG; n + m beyond int32: RENET_ERR_UNSUPPORTED.
 *
 * renet_recurrence_mix_rows: ONE direction per launch.  Row i is the query (ent[i], rel[i], t[i]) with histories as of
 * as_of[i] <= t[i] (device int32 [n]); logits [n, C] with row stride ld (NULL: uniform rows; never written, and not
 * overlapping out); out [n, C] contiguous.  With the sums over the facts (ent, rel, o, t') of the tables with t' < as_of:
 *     w[o]   = sum of 2^(-(t - t') * inv_half_life)          (inv_half_life = 0: plain counts)
 *     W      = sum over o of w[o]
 *     a_i    = alpha if W > 0 else 0      (no history of (ent, rel), or an entity outside [0, num_ent): the prior abstains)
 *     out[o] = log((1 - a_i) * softmax(logits_i)[o] + a_i * w[o] / W)
 * every sum and the logsumexp in fp64, one rounding to fp32 per output, in an order fixed by the table's content: the same
 * bits from run to run, no floating-point atomics.  0 <= alpha < 1, so every output is finite, and a row of out is a
 * normalised log-probability row: renet_rank_rows3 and renet_topk_rows(_wide) read it as they read logits, their row_loss /
 * logp being -log p_mix[gold] / log p_mix.  alpha = 0 gives log_softmax(logits).  A partner outside [0, C) is not addressed.
 * stats / stats_w (both or neither): int32 [n, 2] = (distinct partners seen before as_of, facts counted) and fp32 W [n].
 * C in [1, RENET_RECURRENCE_MAX_C]; alpha outside [0, 1), a negative or non-finite inv_half_life, n < 0, ld < C or a missing
 * array: RENET_ERR_BADARG before any launch; n == 0 is a no-op.  One workgroup per row; no workspace.
 *
 * renet_recurrence_mix_rows_gated: the same kernel body with ONE GATE PER ROW, alpha_row[i] (device fp32 [n], each in [0, 1):
 * the caller's to keep, the entry cannot read it) in the place of alpha -- what a learned per-relation gate is evaluated
 * with.  a_i = alpha_row[i] if W > 0 else 0: a row without history abstains whatever its gate.  A constant alpha_row gives
 * the bits of renet_recurrence_mix_rows.  Refusals as there, and a missing alpha_row.
 *
 * renet_recurrence_gold_rows: what the LOSS through the mix needs of the prior (renet_mix_ce): for row i and the column
 * gold[i] (device int32 [n]),
 *     W[i] = the W of renet_recurrence_mix_rows -- the same strided pass and reduction tree: its stats_w bit for bit
 *     q[i] = fp32(w[gold[i]] / W[i]), both sums in fp64; the gold partner's group is found by binary searches, its counted
 *            facts are those with t' < as_of
 * q = 0 and W = 0 where the pair has no history before as_of or the entity lies outside [0, num_ent); q = 0 where gold lies
 * outside [0, C) or has no counted fact.  One workgroup per row, two floats out, no atomics, no workspace; refusals as for
 * renet_recurrence_mix_rows.
 *
 * renet_recurrence_mix_rows_decay: renet_recurrence_mix_rows_gated with ONE DECAY PER ROW as well, ihl_row[i] (device fp32 [n],
 * each finite and >= 0: the caller's to keep, as alpha_row's range is) in the place of inv_half_life -- what a learned
 * per-relation half-life is evaluated with.  Every weight of row i is 2^(-(t - t') * ihl_row[i]): the strided pass, the
 * per-head sums and the whole-wave sums of long groups read the row's own value.  A constant ihl_row gives the bits of
 * renet_recurrence_mix_rows_gated; rows of one launch do not depend on each other.  A bad decay gives a non-finite row, never
 * an address: it only feeds exp2.  Refusals as there, and a missing ihl_row.
 *
 * renet_recurrence_gold_rows_decay: renet_recurrence_gold_rows with the per-row decay ihl_row[i], and the derivative of q by
 * it.  With the lag D = t - t' of a counted fact and its weight w = 2^(-D * ihl_row[i]),
 *     G = sum over gold's facts of w,  W = sum over all of w,  GD = sum over gold's of D w,  WD = sum over all of D w
 *     q[i]  = fp32(G / W),  W[i] = fp32(W)               (a constant ihl_row: the bits of renet_recurrence_gold_rows)
 *     dq[i] = fp32(-ln2 * (GD * W - G * WD) / (W * W))    = d q / d ihl_row[i];  exactly 0 where W = 0 or G = 0
 * all four sums in fp64 through the same strided shares, shuffle tree and per-wave fold; no atomics: the same bits from run to
 * run.  With L = -log((1 - a) p_g + a q) of renet_mix_ce, dL/dq = -a * exp(L): the loss's gradient reaches the decay as
 * dL/dq * dq.  Three floats out per row; refusals as for renet_recurrence_gold_rows, and a missing ihl_row or dq. */
#define RENET_RECURRENCE_MAX_C (1 << 20)
int renet_pair_append(const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n, const int32_t* ent_ptr,
                      const int32_t* snap_ptr, int n_snaps, const int32_t* ent_ptr_new, const int32_t* snap_ptr_new,
                      int n_snaps_new, int num_ent, const int32_t* new_ent, const int32_t* new_rel, const int32_t* new_other,
                      const int32_t* new_t, int m, int32_t* p_rel_out, int32_t* p_other_out, int32_t* p_t_out, void* stream);
int renet_recurrence_mix_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, int n,
                              const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                              const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, const float* logits,
                              int ld, int C, float alpha, float inv_half_life, float* out, int32_t* stats, float* stats_w,
                              void* stream);
int renet_recurrence_mix_rows_gated(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, int n,
                                    const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                                    const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent,
                                    const float* logits, int ld, int C, const float* alpha_row, float inv_half_life,
                                    float* out, int32_t* stats, float* stats_w, void* stream);
int renet_recurrence_gold_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                               const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t,
                               int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int C,
                               float inv_half_life, float* q, float* W, void* stream);
int renet_recurrence_mix_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, int n,
                                    const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                                    const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent,
                                    const float* logits, int ld, int C, const float* alpha_row, const float* ihl_row,
                                    float* out, int32_t* stats, float* stats_w, void* stream);
int renet_recurrence_gold_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                     const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other,
                                     const int32_t* p_t, int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr,
                                     int n_snaps, int num_ent, int C, const float* ihl_row, float* q, float* W, float* dq,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * RECURRENCE PRIOR FOR EVENT FORECASTS (csrc/joint_mix.hip): the joint copy mix over (relation, entity) pairs -- "s does again
 * what it did before, with whom it did it" mixed into the joint blocks of renet_joint_row_offsets / renet_joint_rank_rows.
 *
 * renet_joint_mix_rows runs AFTER renet_joint_row_offsets on the block scores [G * R, C] (row stride ld) and on off [G * R], IN
 * PLACE.  Group g is one history: the entity ent[g], the query time t[g] and the as_of[g] <= t[g] its window was built with
 * (device int32 [G] each); the pair tables, ent_ptr and snap_ptr are those of the role of the GIVEN entity, as for
 * renet_recurrence_mix_rows.  With the sums over the entity's facts (e, r, c, t') with t' < as_of:
 *     w[r, c] = sum of 2^(-(t - t') * inv_half_life)          (inv_half_life = 0: plain counts)
 *     W       = sum over ALL counted facts of e, every relation              (entity-wide, not per relation)
 *     a       = alpha if W > 0 else 0       (no history, or e outside [0, num_ent): the prior abstains)
 * and J = scores[g * R + r, c] + off[g * R + r], the one fp32 addition of renet_joint_rank_rows, widened to fp64:
 *     M = fp32(J + log1p(-a))                              for a pair without a counted fact
 *     M = fp32(log((1 - a) * exp(J) + a * w[r, c] / W))    for a pair with counted facts
 * For a group with a > 0 the entry writes scores[g * R + r, c] = M and off[g * R + r] = 0: scores + off in one fp32 addition is
 * then M itself, and renet_joint_rank_rows, renet_topk_rows(_wide) + off and renet_select_events read the MIXED joint
 * unchanged.  exp(M) sums to 1 over the R * C pairs where exp(J) does.  A group that abstains keeps its rows and its off
 * untouched, bit for bit; alpha = 0 with W > 0 gives M == J bit for bit (and off = 0).  A fact whose partner lies outside
 * [0, C), or whose relation lies outside [0, R), counts in W and is never addressed.
 * mass [G] (device fp64, the caller's): W of every group, written by a first launch of one workgroup per group and read by
 * the row launch of one workgroup per (g, r) -- W is not summed again in each of the group's R rows.  Every sum is in fp64 in
 * an order fixed by the tables' content and the block size, each output is rounded to fp32 once: no floating-point atomics,
 * the same bits from run to run.  The dense pass is one 16-byte read and one 16-byte write of the row (scalar head and tail:
 * any ld, any row alignment); no workspace.
 * 1 <= R <= 1024, C in [1, RENET_RECURRENCE_MAX_C]; alpha outside [0, 1), a negative or non-finite inv_half_life, ld < C, R or C
 * out of range, G < 0 or a missing array: RENET_ERR_BADARG before any launch; G == 0 is a no-op.
 * Not covered: a gate per relation (with the relation open it gives no normalised joint). */
int renet_joint_mix_rows(const int32_t* ent, const int32_t* t, const int32_t* as_of, int G, const int32_t* p_rel,
                         const int32_t* p_other, const int32_t* p_t, int n_facts, const int32_t* ent_ptr,
                         const int32_t* snap_ptr, int n_snaps, int num_ent, float* scores, int ld, int R, int C, float* off,
                         float alpha, float inv_half_life, double* mass, void* stream);
/* renet_joint_gold_rows: what the LOSS through the joint mix needs of the prior (renet_joint_mix_ce): for row i -- the given
 * entity ent[i], the GOLD relation rel[i], the gold partner gold[i], the query time t[i] and the window as_of[i] (device int32
 * [n] each; tables, ent_ptr and snap_ptr of the given entity's role) -- with w = 2^(-(t - t') * inv_half_life):
 *     G = sum of w over the facts (e, rel, gold, t' < as_of)       W = sum of w over ALL facts (e, *, *, t' < as_of)
 *     q[i] = fp32(G / W),  W[i] = fp32(W)
 * W is the entity-wide W of renet_joint_mix_rows: fp32(mass[g]) of a call on the group (ent, t, as_of), bit for bit (the same
 * strided pass, shuffle tree and wave fold), and exp(-row_loss) of renet_joint_mix_ce is exp(M[rel, gold]) there.
 * q = W = 0 where the entity has no fact before as_of or lies outside [0, num_ent); q = 0 (W kept) where gold lies outside
 * [0, C), rel outside [0, R), or the pair has no counted fact.  One workgroup per row, every sum in fp64 in an order fixed by
 * the tables' content and the block size, one rounding per output: no atomics, no workspace, the same bits from run to run.
 * renet_joint_gold_rows_decay: the decay of row i is ihl_row[i] (device fp32 [n], finite and >= 0: the caller's to keep), and
 * with GD, WD the same two sums of (t - t') w:
 *     dq[i] = fp32(-ln2 (GD W - G WD) / W^2) = d q[i] / d ihl_row[i],  exactly 0 where W = 0 or G = 0
 * (both products rounded separately: q = 1 gives 0).  A constant ihl_row gives the (q, W) of renet_joint_gold_rows bit for bit.
 * 1 <= R <= 1024, C in [1, RENET_RECURRENCE_MAX_C]; R or C out of range, a negative or non-finite inv_half_life, n < 0 or a
 * missing array (ihl_row and dq for the decay entry): RENET_ERR_BADARG before any launch; n == 0 is a no-op. */
int renet_joint_gold_rows(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of, const int32_t* gold,
                          int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t, int n_facts,
                          const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int R, int C,
                          float inv_half_life, float* q, float* W, void* stream);
int renet_joint_gold_rows_decay(const int32_t* ent, const int32_t* rel, const int32_t* t, const int32_t* as_of,
                                const int32_t* gold, int n, const int32_t* p_rel, const int32_t* p_other, const int32_t* p_t,
                                int n_facts, const int32_t* ent_ptr, const int32_t* snap_ptr, int n_snaps, int num_ent, int R,
                                int C, const float* ihl_row, float* q, float* W, float* dq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE builder for the FULL-GRAPH batches of the global model (graph.build_full_graphs; reference Aggregator.py:44-55 /
 * 87-98: dgl.batch of the whole graphs of a list of timestamps).  Resident: the per-timestamp node lists and the facts with
 * LOCAL endpoints (graph.TimeGraph.ent / ls / r / lo, concatenated in graph_dict order).  tidx_dev[G] (device int32,
 * G <= 1024) indexes that order; a repeated index gives two member graphs.  Fills, of RenetBatchOut: seg_ptr, node_ent,
 * row_ptr, col, etype, norm, heavy_rows, e_src, e_dst, chunk_ptr, chunk_type, type_chunk_ptr, it_src, it_type, grp_ptr,
 * plan_*[0] and counts -- bit for bit the arrays of graph.build_full_graphs (tests/test_gpu_full_graph_builder.py).  There is
 * no row prefix (nA = N, n_groups_out = n_groups): node_slot, the *2 arrays, the sequence arrays and plans 1-3 are not
 * touched.  Same protocol as renet_build_batch_both: no host synchronisation, stages launch over the capacities and guard
 * on counts; N > cap_nodes / E > cap_edges set RENET_BB_ERR_NODES / _EDGES, an index outside [0, T) RENET_BB_ERR_TIME, and
 * the batch is then EMPTY (N = E = 0).  N and E follow from node_ptr / trip_ptr, so a caller can size the buffers exactly. */
typedef struct {
    const int32_t* node_ptr;                   /* [T + 1] node range of every timestamp                               */
    const int32_t* node_ent_all;               /* [n_nodes] entity of every node (sorted inside a timestamp)          */
    const int32_t* trip_ptr;                   /* [T + 1] fact range of every timestamp                               */
    const int32_t *trip_ls, *trip_r, *trip_lo; /* [n_facts] local subject, relation, local object                     */
    int T, n_nodes, n_facts, num_ent, num_rels;
} RenetFullStoreDev;

size_t renet_build_full_graphs_workspace(const RenetFullStoreDev* store, int G, int cap_nodes, int cap_edges);
int renet_build_full_graphs(const RenetFullStoreDev* store, const int32_t* tidx_dev, int G, int heavy_thresh,
                            int group_items, int chunk, RenetBatchOut* out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE builder for GROUPED inference batches (graph.build_batch(..., group=...), RGCNAggregator.forward_grouped): ONE
 * direction of B sequences, and sequences of different group ids get SEPARATE member graphs per timestamp -- a slot per
 * (group, timestamp) pair, numbered group-major, then by time.  A batch has thousands of slots, so the node sets are not
 * marked in a [slot][entity] table as in renet_build_batch_both: the 64-bit keys (slot << 32) | entity of every step's
 * subject and history neighbours are radix sorted and numbered (subject keys first, in key order), and the induced edges
 * come from a per-node walk through the store's subject index (graph.GraphStore.subject_index), membership by binary
 * search in the sorted keys.  Per call (device int32, one upload): the batch's s, r, group and its FlatHistory laid out as
 * first / count per sequence, step timestamps, neighbour ranges, neighbours.  idx_dev is the order of the sequences
 * (device int32 [B]); NULL = the order of the arrays, so a caller uploads nothing besides them.  Fills the
 * RenetBatchOut of renet_build_batch_both except rel_label / ent_label (may be NULL), with the row prefix [0, nA) of the
 * subject rows -- bit for bit the arrays of the host builder (tests/test_gpu_grouped_builder.py).  Edge types are stored as
 * type_s: the direction is the kernels' type_shift.  Same protocol: no host synchronisation, stages launch over capacities
 * and guard on counts, RENET_BB_ERR_* in counts[RENET_BB_ERR].  B <= 4096, seq_len <= 32, 2 * num_rels <= 1024. */
typedef struct {
    const int32_t *s, *r, *group;              /* [B] subject, relation row, group id of every sequence               */
    const int32_t *h_first, *h_count;          /* [B] first step and number of steps of every sequence                */
    const int32_t* step_t;                     /* [n_steps] timestamp of every history step                           */
    const int32_t* nbr_ptr;                    /* [n_steps + 1] neighbour range of every step                         */
    const int32_t* nbr_o;                      /* [n_nbr] neighbour entities                                          */
    const int32_t* times;                      /* [T] sorted timestamps of graph_dict                                 */
    const int32_t* trip_ptr;                   /* [T + 1] fact range of every timestamp                               */
    const int32_t *trip_s, *trip_r, *trip_o;   /* [n_facts]                                                           */
    const int32_t* glob_times;                 /* [n_glob] sorted timestamps of the global-embedding table            */
    const int32_t *by_subj, *subj_sorted;      /* [n_facts] facts sorted stably by (timestamp, subject); their subjects */
    int n_steps, n_nbr, T, n_glob, n_facts, num_ent, num_rels;
} RenetGroupedStoreDev;

size_t renet_build_batch_grouped_workspace(const RenetGroupedStoreDev* store, int B, int cap_nodes, int cap_edges);
int renet_build_batch_grouped(const RenetGroupedStoreDev* store, const int32_t* idx_dev, int B, int seq_len,
                              int heavy_thresh, int group_budget, int chunk, const RenetBatchOut* out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * THE MERGED TRAINING STEP AS ONE LAUNCH LIST (round 6; csrc/step.cpp): one iteration of train.py:136-139 --
 *     loss = model(batch, ..., subject=True) + model(batch, ..., subject=False);  loss.backward()
 * on the merged batch of both directions (renet_build_batch_both / graph.build_batch_both) -- issued from C: the forward
 * call enqueues the ~25 launches of  RGCN x2 (RGCN.py:33-51,79-94) -> sequence assembly (Aggregator.py:139-165) -> GRU x2
 * (model.py:86,94) -> both score heads + CE (model.py:89-103), the backward call the ~35 launches of their gradients, on two
 * HIP streams with the fork / join events between them (the relation head and encoder_r's projection next to the entity
 * head / encoder; parameter-gradient kernels that feed nothing but the optimizer on the side stream).  Every launch goes
 * through the entry points of this header with exactly the arguments the Python autograd path (re-net_amd/ops.py) passes,
 * so losses and gradients are BIT-identical to that path (tests/test_gpu_step_plan.py); the host cost of a step drops from
 * ~55 Python-level C-ABI calls to two.
 *   RenetStepModel : parameters and their gradient buffers (gradients ACCUMULATE: beta = 1 everywhere, as into an existing
 *                    .grad), the global-embedding matrix, optionally the planes of the entity head's weight
 *   RenetStepBatch : the device arrays of one merged batch (graph.DeviceGraph / gpu_builder.DeviceBatch) + its sizes
 *   RenetStepRun   : dropout seeds, loss scales, the workspace, the two streams
 *   renet_step_workspace : bytes of workspace for (model, batch); activations live there between forward and backward
 *   renet_step_forward   : writes the 2 B per-row losses (entity head rows, then relation head rows) to row_loss
 *   renet_step_backward  : upstream scalar g (device); defer_side != 0 leaves the side stream UN-joined (the caller joins it
 *                          before it reads a parameter gradient: parallel.HipAdam.step); ev_head_done (optional hipEvent_t)
 *                          is recorded when the entity head's weight / bias gradients are complete (early all-reduce bucket),
 *                          ev_gru_done (optional) when both encoders' parameter gradients are (the middle bucket)
 *   both return the number of C-ABI launches they issued in *n_launches (optional).
 *   RENET_STEP_BATCH (environment, read once; default 22; renet_step_batch_mask() returns it): bit 2 = the head's and the
 *   sequence assembly's segmented adds as one renet_segment_add_multi launch, bit 4 = the W_hh splits issued early on the
 *   side stream (renet_gru_split_weights), bit 16 = a stale head weight (lin_w_stale; lin_w_planes is then the buffer
 *   renet_step_forward fills) is packed on the side stream beside the forward recurrence instead of at the top of the main
 *   stream; bits 1 and 8 are not assigned; 0 = one launch per sum, the splits inside the GRU calls.  Same bits of every
 *   result either way.
 * fp32-class default mode only (bf16x6 GEMMs, bf16x6 recurrences); tensors below 2 GiB. */
typedef struct { const int32_t *order, *seg_ptr, *target; int num_segments; } RenetSegPlan;
typedef struct {
    int D, num_ent, T, C2;                     /* n_hidden; entities; 2 * num_rels relation types; classes of the relation head */
    float drop_p;                              /* 0 in eval mode */
    const float *ent, *rel;                    /* [num_ent, D], [T, D] */
    const float *w1, *loop1, *w2, *loop2;      /* rgcn1 / rgcn2: weight [T, D * D / 100], loop_weight [D, D] */
    const float *wih, *whh, *bih, *bhh;        /* encoder   (4D -> D): [3D, 4D], [3D, D], [3D], [3D] */
    const float *wih_r, *whh_r, *bih_r, *bhh_r;/* encoder_r (3D -> D): [3D, 3D], ... */
    const float *lin_w, *lin_b;                /* linear   [num_ent, 3D], [num_ent] */
    const float *linr_w, *linr_b;              /* linear_r [C2, 2D], [C2] */
    float *g_ent, *g_rel, *g_w1, *g_loop1, *g_w2, *g_loop2, *g_wih, *g_whh, *g_bih, *g_bhh, *g_wih_r, *g_whh_r, *g_bih_r,
          *g_bhh_r, *g_lin_w, *g_lin_b, *g_linr_w, *g_linr_b;
    const float* glob;                         /* [n_glob, D] global embeddings (a constant of the step) */
    const void* lin_w_planes;                  /* optional: renet_pack_planes(lin_w); NULL = the in-loop-split head */
    size_t lin_w_plane;                        /*   elements per plane */
    int lin_w_ld;                              /*   Cp of the planes */
    int lin_w_stale;                           /* != 0: the planes are older than lin_w; renet_step_forward packs them */
} RenetStepModel;
typedef struct {
    int N, E, nA, S, B, L, n_items;            /* nodes, edges, rows of layer 2, packed rows, sequences, steps, items */
    int n_groups, n_groups_out, n_heavy, n_heavy_out, n_chunks, n_chunks2;
    const int32_t* step_off_host;              /* [L + 1] HOST copy of step_off */
    const int32_t *node_ent, *row_ptr, *col, *etype;
    const float* norm;
    const int32_t *it_src, *it_type, *grp_ptr, *heavy_rows, *heavy_rows_out;
    const int32_t *it_src_t, *it_type_t, *col_t, *e_src_t;        /* renet_compose_table_items */
    const int32_t *e_src, *e_dst, *chunk_ptr, *chunk_type, *type_chunk_ptr;
    const int32_t *e_src2, *e_dst2, *chunk_ptr2, *chunk_type2, *type_chunk_ptr2;
    const int32_t *subj_row, *row_ent, *row_rel, *glob_row, *step_off;
    const int32_t *s_idx, *r_idx, *ent_label, *rel_label;
    RenetSegPlan plan_node_ent, plan_subj_row, plan_s, plan_r;
} RenetStepBatch;
typedef struct {
    uint64_t seed_rgcn1, seed_rgcn2, seed_x, seed_xr, seed_head1, seed_head2;
    float scale_ent, scale_rel;                /* CE gradient scales: loss_scale / B and loss_scale * 0.1 / B (model.py:103) */
    void* workspace;
    size_t workspace_bytes;
    void *stream, *side_stream;                /* hipStream_t; side_stream may equal stream (everything in stream order) */
} RenetStepRun;
size_t renet_step_workspace(const RenetStepModel* m, const RenetStepBatch* b);
int renet_step_forward(const RenetStepModel* m, const RenetStepBatch* b, const RenetStepRun* r, float* row_loss,
                       int* n_launches);
int renet_step_backward(const RenetStepModel* m, const RenetStepBatch* b, const RenetStepRun* r, const float* g,
                        int defer_side, void* ev_head_done, void* ev_gru_done, int* n_launches);
int renet_step_batch_mask(void);
/* x[0..n) += y[0..n) (the two heads' gradients wrt the same gathered rows ent[s], model.py:89,98, before ONE scatter-add) */
int renet_add_inplace(float* x, const float* y, size_t n, void* stream);
/* x[0..n) = 0 as an ordinary kernel launch (the zero-initialised scatter-add targets of the backward pass: hipMemsetAsync goes
 * through the runtime's blit path, whose packets do not pipeline with the neighbouring kernel dispatches) */
int renet_zero(float* x, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HOST-side batch-graph builder passes (no device work; pointers are HOST arrays): the native form of
 * graph.build_batch's heavy middle, replacing the reference's per-batch DGL subgraph/batch calls
 * (utils.py:115-131,158-170,236-241).  See csrc/host_builder.cpp for the contracts. */
int64_t renet_host_filter_edges(const int64_t* trip_ptr, const int64_t* trip_s, const int64_t* trip_r,
                                const int64_t* trip_o, const int64_t* ti, int64_t Tb, int64_t num_ent,
                                const int64_t* keys, const int32_t* new_id, int64_t N, int32_t* table,
                                int64_t* out_ls, int64_t* out_lo, int64_t* out_rr);
/* The same result for MANY small member graphs (batched inference: one slot per (entity, timestamp)): walks only
 * the facts whose subject is in the slot's node set through a per-timestamp subject index -- by_subj = fact
 * indices sorted stably by (timestamp, subject), subj_sorted = their subjects; `table`: num_ent entries, -1. */
int64_t renet_host_filter_edges_sparse(const int64_t* trip_ptr, const int64_t* trip_s, const int64_t* trip_r,
                                       const int64_t* trip_o, const int64_t* by_subj,
                                       const int64_t* subj_sorted, const int64_t* ti, int64_t Tb,
                                       int64_t num_ent, const int64_t* keys, const int32_t* new_id, int64_t N,
                                       int32_t* table, int64_t* out_ls, int64_t* out_lo, int64_t* out_rr);
/* The relation-bucketed chunk list of renet_host_edge_layouts restricted to edges with dst < n_out (a layer
 * evaluated on a row prefix); returns the number of kept edges. */
int64_t renet_host_type_chunks(int64_t E, const int64_t* src, const int64_t* dst, const int64_t* et, int64_t T,
                               int64_t chunk, int64_t n_out, int32_t* e_src, int32_t* e_dst,
                               int32_t* type_chunk_ptr, int32_t* chunk_type, int32_t* chunk_ptr,
                               int64_t* n_chunks);
/* Node sets of a batch (utils.py:149-156) -- per member graph the union of the subjects and history objects of its
 * steps -- as sorted keys slot * num_ent + entity, with the rows that are some step's subject numbered first
 * (graph.build_batch documents the outputs); `table`: num_ent entries, -1.  Returns the number of nodes. */
int64_t renet_host_node_sets(int64_t S, const int64_t* slot_k, const int64_t* subj_ent, const int64_t* nbr_begin,
                             const int64_t* nbr_cnt, const int64_t* nbr_o, int64_t Tb, int64_t num_ent,
                             int32_t* table, int64_t* keys, int64_t* subj_pos, int64_t* new_id,
                             int32_t* node_ent, int64_t* node_slot, int64_t* n_a);
void renet_host_edge_layouts(int64_t n, int64_t E, const int64_t* src, const int64_t* dst, const int64_t* et,
                             int64_t T, int64_t chunk, int64_t heavy, int32_t* col, int32_t* etype,
                             int32_t* row_ptr, float* norm, int32_t* heavy_rows, int64_t* n_heavy,
                             int32_t* e_src, int32_t* e_dst, int32_t* type_chunk_ptr, int32_t* chunk_type,
                             int32_t* chunk_ptr, int64_t* n_chunks);
int64_t renet_host_segplan(const int64_t* idx, int64_t n, int64_t bound, int32_t* order, int32_t* seg_ptr,
                           int32_t* target);
/* Item stream + wave groups consumed by renet_rgcn_gather_items, from the CSR of renet_host_edge_layouts (its
 * contract is stated there and in graph.plan_gather_items, the numpy specification).  Capacities: it_src / it_type
 * E + N, grp_ptr N + 2.  Returns the number of groups, or -1 if budget + heavy + 1 > 64. */
int64_t renet_host_gather_items(int64_t N, const int32_t* row_ptr, const int32_t* col, const int32_t* etype,
                                int64_t heavy, int64_t budget, int64_t n_out, int32_t* it_src, int32_t* it_type,
                                int32_t* grp_ptr, int64_t* n_items, int64_t* n_groups_out);

#ifdef __cplusplus
}
#endif
#endif /* RENET_HIP_H */
