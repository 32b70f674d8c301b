"""ctypes binding of librenet_hip.so (include/renet_hip.h).  PyTorch-ROCm is only the owner of device
memory and streams here: every function takes torch CUDA(HIP) tensors, checks dtype/contiguity,
and passes raw device pointers + the current stream to the C ABI.

There is NO fallback: if the library is missing or a call fails, this raises.
"""
import contextlib
import ctypes
import functools
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RENET_HIP_LIB', os.path.join(_HERE, 'csrc', 'librenet_hip.so'))   # env: A/B builds

_lib = None

c_int = ctypes.c_int
c_float = ctypes.c_float
c_void_p = ctypes.c_void_p
c_size_t = ctypes.c_size_t
c_u64 = ctypes.c_uint64

# argument lists that several entry points share verbatim
_GEMM_ARGS = [c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_int,
              c_float, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]
_RGCN_BWD_W_ARGS = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                    c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_size_t, c_void_p]
_GRU_FWD_LAYOUTS_ARGS = [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
_GRU_BWD_LAYOUTS_ARGS = [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_size_t, c_void_p]

_SIGNATURES = {
    'renet_version': (c_int, []),
    'renet_gather_rows': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'renet_segment_add': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'renet_segment_add2': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    'renet_segment_add_multi': (c_int, [c_int, c_void_p, c_int, c_void_p]),
    'renet_step_batch_mask': (c_int, []),
    'renet_gru_split_weights': (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    'renet_gru_fwd_layouts_presplit': (c_int, _GRU_FWD_LAYOUTS_ARGS),
    'renet_gru_bwd_layouts_presplit': (c_int, _GRU_BWD_LAYOUTS_ARGS),
    'renet_rgcn_gather': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_int, c_int, c_void_p, c_float, c_u64, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_int, c_int, c_int, c_void_p]),
    'renet_rgcn_gather_items': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_u64,
                                        c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'renet_rgcn_gather_items_bf16': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                             c_float, c_u64, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                             c_int, c_void_p]),
    'renet_rgcn_gather_items_table_bf16': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                   c_int, c_int, c_void_p, c_float, c_u64, c_int, c_void_p, c_int,
                                                   c_void_p, c_int, c_void_p]),
    'renet_rgcn_gather_items_table': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                              c_float, c_u64, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    'renet_compose_table_items': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_rgcn_bwd_prep': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_u64, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p]),
    'renet_rgcn_bwd_prep_bounds': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_u64, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_bound_parts': (c_int, [c_size_t]),
    'renet_rgcn_bwd_w_workspace': (c_size_t, [c_int, c_int]),
    'renet_rgcn_bwd_w': (c_int, _RGCN_BWD_W_ARGS),
    'renet_rgcn_bwd_w64': (c_int, _RGCN_BWD_W_ARGS),
    'renet_gemm_workspace': (c_size_t, [c_int, c_int, c_int]),
    'renet_gemm_f32': (c_int, _GEMM_ARGS),
    'renet_gemm_f32_split': (c_int, _GEMM_ARGS),
    'renet_gemm_bf16': (c_int, _GEMM_ARGS),
    'renet_gemm_split_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    'renet_maxabs_blocks': (c_int, [c_int, c_int, c_int]),
    'renet_maxabs_partials_multi': (c_int, [c_void_p, c_int, c_void_p]),
    'renet_maxabs_partials': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'renet_gemm_f32_h3': (c_int, [c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_int,
                                  c_float, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int,
                                  c_void_p, c_int, c_void_p]),
    'renet_bf16_bytes': (c_size_t, [c_int, c_int]),
    'renet_pack_bf16': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'renet_gemm_bf16s': (c_int, _GEMM_ARGS),
    'renet_bf16_zero_padding': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'renet_seq_assemble_fwd_bf16': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int, c_int, c_float, c_u64, c_u64, c_void_p, c_int, c_void_p,
                                            c_int, c_int, c_void_p]),
    'renet_softmax_ce_bf16': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int,
                                      c_void_p]),
    'renet_gru_bwd_layouts_bf16out': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'renet_colsum_bf16': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
    'renet_scale_bf16_by_device_scalar': (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    'renet_planes_elems': (c_size_t, [c_int, c_int]),
    'renet_pack_planes': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'renet_gemm_planes': (c_int, [c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_size_t,
                                  c_void_p, c_int, c_size_t, c_float, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                  c_void_p, c_size_t, c_void_p]),
    'renet_softmax_ce_planes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t,
                                        c_int, c_int, c_void_p]),
    'renet_step_workspace': (c_size_t, [c_void_p, c_void_p]),
    'renet_step_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_step_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'renet_add_inplace': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    'renet_zero': (c_int, [c_void_p, c_size_t, c_void_p]),
    'renet_colsum_workspace': (c_size_t, [c_int, c_int]),
    'renet_colsum': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
    'renet_scale_by_device_scalar': (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    'renet_scale_by_device_scalar_bound': (c_int, [c_void_p, c_size_t, c_void_p, c_float, c_void_p, c_void_p]),
    'renet_seq_assemble_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_int, c_float, c_u64, c_u64, c_void_p, c_void_p,
                                       c_void_p]),
    'renet_seq_assemble_fwd_bounds': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int, c_int, c_float, c_u64, c_u64, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
    'renet_seq_assemble_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                       c_u64, c_u64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_gru_workspace': (c_size_t, [c_int, c_int]),
    'renet_gru_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                              c_void_p, c_size_t, c_void_p]),
    'renet_gru_bwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_size_t, c_void_p]),
    'renet_gru_fwd_multi': (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'renet_gru_bwd_multi': (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    'renet_gru_fwd_layouts': (c_int, _GRU_FWD_LAYOUTS_ARGS),
    'renet_gru_bwd_layouts': (c_int, _GRU_BWD_LAYOUTS_ARGS),
    'renet_gru_bound_parts': (c_int, [c_int]),
    'renet_gru_bwd_layouts_bounds': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'renet_gru_fwd_layouts_f32': (c_int, _GRU_FWD_LAYOUTS_ARGS),
    'renet_gru_bwd_layouts_f32': (c_int, _GRU_BWD_LAYOUTS_ARGS),
    'renet_gru_fwd_layouts_bf16': (c_int, _GRU_FWD_LAYOUTS_ARGS),
    'renet_gru_bwd_layouts_bf16': (c_int, _GRU_BWD_LAYOUTS_ARGS),
    'renet_concat3_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                                  c_u64, c_void_p, c_void_p]),
    'renet_concat3_fwd_bounds': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                                         c_u64, c_void_p, c_void_p, c_void_p]),
    'renet_concat3_bwd': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_u64, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    'renet_dropout': (c_int, [c_void_p, c_size_t, c_float, c_u64, c_void_p, c_void_p]),
    'renet_softmax_ce': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                 c_void_p]),
    'renet_soft_ce_sparse': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                     c_void_p, c_void_p]),
    'renet_joint_softmax': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'renet_rank_rows': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    'renet_rank_rows3': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                 c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'renet_topk_rows': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_topk_rows_wide_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'renet_topk_rows_wide': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'renet_joint_row_offsets': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'renet_joint_rank_rows': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    'renet_select_events_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'renet_select_events': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 12 + [c_void_p, c_size_t, c_void_p]),
    'renet_topk_workspace': (c_size_t, [c_int]),
    'renet_topk_positive': (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    'renet_build_batch_workspace': (c_size_t, [c_void_p, c_int, c_int, c_int]),
    'renet_build_batch_both': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    'renet_query_histories': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p]),
    'renet_store_append_workspace': (c_size_t, [c_int, c_int]),
    'renet_store_append': (c_int, [c_void_p] * 7 + [c_int] * 4 + [c_void_p] * 4 + [c_int, c_int] + [c_void_p] * 8
                           + [c_size_t, c_void_p]),
    'renet_append_i32': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'renet_pair_append': (c_int, [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int]
                          + [c_void_p] * 4 + [c_int] + [c_void_p] * 4),
    'renet_recurrence_mix_rows': (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int,
                                          c_void_p, c_int, c_int, c_float, c_float] + [c_void_p] * 4),
    'renet_recurrence_mix_rows_gated': (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int,
                                                c_int, c_void_p, c_int, c_int, c_void_p, c_float] + [c_void_p] * 4),
    'renet_recurrence_gold_rows': (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int,
                                           c_int, c_float] + [c_void_p] * 3),
    'renet_recurrence_mix_rows_decay': (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int,
                                                c_int, c_void_p, c_int, c_int, c_void_p, c_void_p] + [c_void_p] * 4),
    'renet_recurrence_gold_rows_decay': (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int,
                                                 c_int, c_int, c_void_p] + [c_void_p] * 4),
    'renet_joint_mix_rows': (c_int, [c_void_p] * 3 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    'renet_joint_gold_rows': (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_int, c_float] + [c_void_p] * 3),
    'renet_joint_gold_rows_decay': (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int,
                                            c_int, c_int, c_void_p] + [c_void_p] * 4),
    'renet_joint_mix_ce': (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_float] + [c_void_p] * 5),
    'renet_joint_mix_ce_planes': (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_int,
                                          c_int, c_void_p, c_void_p, c_void_p]),
    'renet_mix_ce': (c_int, [c_void_p] * 4 + [c_int, c_int, c_int, c_float] + [c_void_p] * 4),
    'renet_mix_ce_planes': (c_int, [c_void_p] * 4 + [c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_int, c_int,
                                    c_void_p, c_void_p]),
    'renet_build_full_graphs_workspace': (c_size_t, [c_void_p, c_int, c_int, c_int]),
    'renet_build_full_graphs': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    'renet_build_batch_grouped_workspace': (c_size_t, [c_void_p, c_int, c_int, c_int]),
    'renet_build_batch_grouped': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    'renet_adam_workspace': (c_size_t, [c_size_t]),
    'renet_adam_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float,
                                c_float, c_float, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'renet_adam_step_scaled': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float,
                                       c_float, c_float, c_float, c_float, c_int, c_int, c_void_p, c_size_t, c_void_p,
                                       c_void_p]),
    'renet_sumsq_partials': (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    'renet_adam_step_presummed': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float,
                                          c_float, c_float, c_float, c_float, c_int, c_int, c_void_p, c_int, c_void_p,
                                          c_void_p]),
    'renet_host_filter_edges': (ctypes.c_int64, [c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p,
                                                 ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_host_filter_edges_sparse': (ctypes.c_int64, [c_void_p] * 7 + [ctypes.c_int64, ctypes.c_int64, c_void_p,
                                                        c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p,
                                                        c_void_p]),
    'renet_host_node_sets': (ctypes.c_int64, [ctypes.c_int64] + [c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int64]
                             + [c_void_p] * 7),
    'renet_host_type_chunks': (ctypes.c_int64, [ctypes.c_int64, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int64] + [c_void_p] * 6),
    'renet_host_edge_layouts': (None, [ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                       ctypes.c_int64, ctypes.c_int64] + [c_void_p] * 12),
    'renet_host_segplan': (ctypes.c_int64, [c_void_p, ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p, c_void_p]),
    'renet_host_gather_items': (ctypes.c_int64, [ctypes.c_int64, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                                 ctypes.c_int64, ctypes.c_int64] + [c_void_p] * 5),
    'renet_segment_pool_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'renet_segment_pool_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p]),
    'renet_nbr_pool_fwd': (c_int, [c_void_p] * 12 + [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'renet_nbr_pool_bwd': (c_int, [c_void_p] * 12 + [c_int, c_int, c_int] + [c_void_p] * 7),
}

EXPORTS = sorted(_SIGNATURES)


class RenetHipError(RuntimeError):
    pass


class _Bound(object):
    """The bound entry points (attribute per symbol)."""


def _exact_arity(fn, name, n):
    # ctypes silently accepts EXTRA positional arguments and converts them as 32-bit ints (a pointer passed
    # that way is truncated): insist on the declared arity
    def call(*a):
        if len(a) != n:
            raise RenetHipError('%s takes %d arguments, %d given' % (name, n, len(a)))
        return fn(*a)
    call.__name__ = name
    return call


def lib():
    """Loads librenet_hip.so (once).  Raises if it has not been built -- no CPU/torch fallback."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RenetHipError('librenet_hip.so not built (%s); run `python re-net_amd/build.py` '
                                '-- there is no fallback path' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        ns = _Bound()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(ns, name, _exact_arity(fn, name, len(args)))
        if ns.renet_version() != 1:
            raise RenetHipError('ABI version mismatch')
        ns._cdll = L
        _lib = ns
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RenetHipError('%s failed with code %d' % (what, rc))


def _dev_ptr(dtype, default_name, t, name=None):
    """Device address of the contiguous tensor t of `dtype` (None stays None)."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RenetHipError('%s must be a contiguous %s device tensor' % (name or default_name, str(dtype)[6:]))
    return t.data_ptr()


_f32 = functools.partial(_dev_ptr, torch.float32, 'tensor')        # _f32(t, name='tensor')
_i32 = functools.partial(_dev_ptr, torch.int32, 'index')           # _i32(t, name='index')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """Handle of torch's CURRENT stream on the current device (the stream every C-ABI call launches on).  Through the raw
    accessor when this torch has it: `torch.cuda.current_stream()` builds a Python Stream object per call (~12 us, 50+ times
    per training step: a quarter of the thread time a step needs to enqueue, tools/host_profile.py)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-kernel-class timing with HIP events on the launch stream (bench.py) -----------
class KernelTimer(object):
    """Collects (start, stop) HIP events around C-ABI calls plus the ALGORITHMIC work of each call.
    torch.cuda.Event records on torch's current stream, which is the stream the call launches on."""

    def __init__(self):
        self.recs = {}

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, e0, flops=0.0, nbytes=0.0, tag=None):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.recs.setdefault(name, []).append((e0, e1, flops, nbytes, tag))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, rs in self.recs.items():
            out[name] = {'calls': len(rs), 'ms': sum(r[0].elapsed_time(r[1]) for r in rs),
                         'flops': sum(r[2] for r in rs), 'bytes': sum(r[3] for r in rs)}
        return out

    def by_tag(self, name):
        """per-tag breakdown of one class (GEMMs: tag = (ta, tb, m, n, k, split_k))"""
        torch.cuda.synchronize()
        out = {}
        for r in self.recs.get(name, []):
            o = out.setdefault(r[4], {'calls': 0, 'ms': 0.0, 'flops': 0.0})
            o['calls'] += 1
            o['ms'] += r[0].elapsed_time(r[1])
            o['flops'] += r[2]
        return out


_timer = None


def _timed():
    """Start of a timed library call: the start event, None while no timer is installed.  Every wrapper with a timer class
    of its own brackets its call with _timed() / _timed_end()."""
    return _timer.begin() if _timer is not None else None


def _timed_end(t0, name, flops=0.0, nbytes=0.0, tag=None):
    if t0 is not None:
        _timer.end(name, t0, flops=flops, nbytes=nbytes, tag=tag)

# wrappers without a timer of their own (the step's small kernels): set_timer(t, glue=True) times each of them as class
# 'glue:<name>' so that bench.py's `kernel_only` covers EVERY C-ABI launch of a step, not only the named classes
GLUE = ('softmax_ce_planes', 'gather_rows', 'segment_add', 'segment_add2', 'compose_table_items', 'rgcn_bwd_prep', 'colsum',
        'scale_by_device_scalar', 'seq_assemble_fwd', 'seq_assemble_fwd_bf16', 'softmax_ce_bf16', 'seq_assemble_bwd',
        'concat3_fwd', 'concat3_bwd', 'dropout', 'softmax_ce', 'adam_step', 'segment_pool_fwd', 'segment_pool_bwd',
        'pack_bf16_glue', 'soft_ce_sparse', 'mix_ce', 'mix_ce_planes', 'joint_mix_ce', 'joint_mix_ce_planes')
_glue_saved = {}


def _timed_glue(name, fn):
    @functools.wraps(fn)
    def call(*a, **k):
        t = _timer
        if t is None:
            return fn(*a, **k)
        e0 = t.begin()
        try:
            return fn(*a, **k)
        finally:
            t.end('glue:' + name, e0)
    return call


def set_timer(t, glue=False):
    """Installs (None: removes) the kernel timer.  glue=True also times the wrappers listed in GLUE."""
    global _timer
    _timer = t
    g = globals()
    for name, fn in _glue_saved.items():
        g[name] = fn
    _glue_saved.clear()
    if t is not None and glue:
        for name in GLUE:
            if name in g and callable(g[name]):
                _glue_saved[name] = g[name]
                g[name] = _timed_glue(name, g[name])


# ---- thin typed wrappers -----------------------------------------------------------------------
def gather_rows(table, idx, out=None):
    n, d = idx.numel(), table.shape[1]
    if out is None:
        out = torch.empty(n, d, device=table.device, dtype=torch.float32)
    _check(lib().renet_gather_rows(_f32(table), _i32(idx), n, d, _f32(out), _stream()), 'gather_rows')
    return out


def segment_add(src, plan, dst):
    """dst[plan.target[u]] += sum of src rows listed in plan (deterministic)."""
    _check(lib().renet_segment_add(_f32(src), _i32(plan.order), _i32(plan.seg_ptr), _i32(plan.target),
                                   plan.num_segments, src.shape[1], _f32(dst), _stream()), 'segment_add')
    return dst


def segment_add2(src0, src1, plan, dst0, dst1):
    """dst0[target] += segment sums of src0 and dst1[target] += segment sums of src1, one launch, one plan."""
    _check(lib().renet_segment_add2(_f32(src0), _f32(src1), _i32(plan.order), _i32(plan.seg_ptr), _i32(plan.target),
                                    plan.num_segments, src0.shape[1], _f32(dst0), _f32(dst1), _stream()), 'segment_add2')


class SegAddJobC(ctypes.Structure):
    """RenetSegAddJob"""
    _fields_ = [('order', c_void_p), ('seg_ptr', c_void_p), ('seg_target', c_void_p), ('U', c_int), ('dst', c_void_p),
                ('dst_rows', c_int), ('overwrite', c_int), ('a0', c_void_p), ('a1', c_void_p), ('b', c_void_p)]


def segment_add_multi(jobs):
    """jobs: up to 4 of (plan, dst, a0, a1 | None, b | None, overwrite) -- per job dst[target] (+)= segment sums of a0 (+ a1),
    then of b, in ONE launch (renet_segment_add_multi); -> the library's return code."""
    arr = (SegAddJobC * max(len(jobs), 1))()
    d = 0
    for j, (plan, dst, a0, a1, b, overwrite) in zip(arr, jobs):
        j.order, j.seg_ptr, j.seg_target, j.U = _i32(plan.order), _i32(plan.seg_ptr), _i32(plan.target), plan.num_segments
        j.dst, j.dst_rows, j.overwrite = _f32(dst), dst.shape[0], int(bool(overwrite))
        j.a0, j.a1, j.b = _f32(a0), _f32(a1), _f32(b)
        d = dst.shape[1]
    return lib().renet_segment_add_multi(len(jobs), ctypes.addressof(arr), d, _stream())


def gru_split_weights(w_hhs, hdim, backward, ws, ws_bytes):
    """The W_hh plane split of gru_fwd_layouts (backward=False) / gru_bwd_layouts (True) into the slots of `ws`, on the current
    stream (renet_gru_split_weights); -> the library's return code."""
    return lib().renet_gru_split_weights(len(w_hhs), _ptrs(w_hhs), hdim, int(bool(backward)), ws.data_ptr(), ws_bytes,
                                         _stream())


def _heavy(rows):
    """(pointer, count) of a hub-row list; (None, 0) without one."""
    return (_i32(rows), rows.numel()) if rows is not None else (None, 0)


def _gather_timed_end(t0, name, n_edges, n_rows, d, weight, has_addend, x_bytes=4, w_bytes=4):
    """The timer record of one gather launch: nbytes = its algorithmic bytes, tag = the strict bytes (no addend row)."""
    if t0 is not None:
        _timed_end(t0, name, nbytes=float(gather_bytes(n_edges, n_rows, d, weight.numel(), has_addend, x_bytes, w_bytes)),
                   tag=float(gather_bytes(n_edges, n_rows, d, weight.numel(), False, x_bytes, w_bytes)))


def rgcn_gather(x, row_ptr, col, etype, scale, weight, type_shift, transpose_w, addend, drop_p, seed,
                relu, out, heavy_rows=None, heavy_thresh=0, src_limit=0, addend_rows=0, n_edges=None):
    """n_edges: edges actually walked by this launch (pruned launches), for the byte accounting only."""
    d = x.shape[1]
    t0 = _timed()
    _check(lib().renet_rgcn_gather(_f32(x), d, _i32(row_ptr), _i32(col), _i32(etype), _f32(scale),
                                   _f32(weight), weight.shape[0], type_shift, int(transpose_w),
                                   _f32(addend), float(drop_p), int(seed), int(relu), _f32(out),
                                   out.shape[0], *_heavy(heavy_rows), int(heavy_thresh),
                                   int(src_limit), int(addend_rows), _stream()), 'rgcn_gather')
    if t0 is not None:
        # launches over the full batch graph (layer 1 and its backward) and the pruned ones (last layer:
        # subject rows only, a few thousand short rows -- launch-latency bound) are different regimes
        e = col.numel() if n_edges is None else int(n_edges)
        _timed_end(t0, 'rgcn_gather' if n_edges is None else 'rgcn_gather_pruned',
                   nbytes=float(gather_bytes(e, out.shape[0], d, weight.numel(), addend is not None)))
    return out


def gather_bytes(n_edges, n_rows, d, weight_numel, has_addend, x_bytes=4, w_bytes=4):
    """Algorithmic bytes of one gather-SpMM launch: per edge one source row + its source and type
    index; per output row the row itself + row_ptr + norm (+ the fused self-loop addend row, which the formula
    allows to count when the epilogue is fused); the relation weight table once.  x_bytes / w_bytes: element size
    of the source rows / the relation table as STORED (2 in the bf16-storage forms)."""
    return (n_edges * (d * x_bytes + 8) + n_rows * (d * 4 + 8) + weight_numel * w_bytes +
            (n_rows * d * 4 if has_addend else 0))


def _item_args(it_src, it_type, g, n_groups, col):
    """The argument run every item entry has behind D: the item stream, then the CSR arrays the hub rows walk."""
    return (_i32(it_src), _i32(it_type), _i32(g.grp_ptr), int(n_groups), _i32(g.row_ptr), _i32(col), _i32(g.etype))


def rgcn_gather_items(x, g, weight, type_shift, transpose_w, addend, drop_p, seed, relu, out, use_norm=True,
                      pruned=False, src_limit=0, addend_rows=0, w16=None):
    """renet_rgcn_gather_items on the planned item stream of DeviceGraph `g` (graph.plan_gather_items).
    pruned: the launch covers the row prefix [0, out.shape[0]) = g.nA (groups / hub rows of that prefix) in the
    forward, or all rows with the edges whose source is >= src_limit skipped in the backward.
    w16: the bf16 copy of `weight` (gather_weight_bf16; bf16-storage mode) -- the relation blocks are then read as bf16."""
    d = x.shape[1]
    n_rows = out.shape[0]
    prefix = n_rows < g.N
    n_groups = g.n_groups_out if prefix else g.n_groups
    heavy = g.heavy_rows_out if prefix else g.heavy_rows
    if max(x.numel(), out.numel()) * 4 >= (1 << 31):
        # the item kernels address with 32-bit buffer offsets (< 2 GiB per tensor: 2.6 M rows at D = 200); beyond
        # that the plain-CSR kernel with 64-bit addressing takes over
        return rgcn_gather(x, g.row_ptr, g.col, g.etype, g.norm if use_norm else None, weight, type_shift,
                           transpose_w, addend, drop_p, seed, relu, out, heavy, g.heavy_thresh, src_limit,
                           addend_rows, n_edges=g.E_out if pruned else None)
    t0 = _timed()
    head = (_f32(x), d) + _item_args(g.it_src, g.it_type, g, n_groups, g.col) + (_f32(g.norm) if use_norm else None,)
    tail = (weight.shape[0], int(type_shift), int(transpose_w), _f32(addend), float(drop_p), int(seed), int(relu),
            _f32(out), n_rows) + _heavy(heavy) + (int(src_limit), int(addend_rows), int(pruned), _stream())
    if w16 is not None:
        _check(lib().renet_rgcn_gather_items_bf16(*head, w16.p.data_ptr(), w16.p.shape[1], *tail),
               'rgcn_gather_items_bf16')
    else:
        _check(lib().renet_rgcn_gather_items(*head, _f32(weight), *tail), 'rgcn_gather_items')
    _gather_timed_end(t0, 'rgcn_gather_%s_%s' % ('bwdh' if transpose_w else 'fwd', 'pruned' if pruned else 'full'),
                      g.E_out if pruned else g.E, n_rows, d, weight, addend is not None, 4, 2 if w16 is not None else 4)
    return out


def gather_weight_bf16(weight):
    """bf16 copy of an fp32 matrix the gather kernels read (the relation-block table, the entity table) in
    bf16-storage mode, else None.  Registered weights come from the per-optimizer-step cache (_as_bf16).
    RENET_BF16_GATHER=0 keeps the gathers on fp32 operands."""
    if current_mode() != 'bf16s' or os.environ.get('RENET_BF16_GATHER', '1') == '0':
        return None
    if weight.numel() * 2 >= (1 << 31):
        return None
    return _as_bf16(weight)[0]


def compose_table_items(g):
    """Index arrays of the table-addressed first layer for DeviceGraph `g` (renet_compose_table_items): source rows
    composed through g.node_ent.  -> (it_src_t, it_type_t, col_t, e_src_t), int32 device tensors."""
    ni, e = g.it_src.numel(), g.col.numel()
    buf = torch.empty(2 * ni + 2 * e + 16, device=g.col.device, dtype=torch.int32)
    a0, a1, a2 = (ni + 3) & ~3, 2 * ((ni + 3) & ~3), 2 * ((ni + 3) & ~3) + ((e + 3) & ~3)
    it_src_t, it_type_t, col_t, e_src_t = buf[:ni], buf[a0:a0 + ni], buf[a1:a1 + e], buf[a2:a2 + e]
    _check(lib().renet_compose_table_items(_i32(g.node_ent), _i32(g.it_src), _i32(g.it_type), ni, _i32(g.col),
                                           _i32(g.e_src), e, it_src_t.data_ptr(), it_type_t.data_ptr(),
                                           col_t.data_ptr(), e_src_t.data_ptr(), _stream()), 'compose_table_items')
    return it_src_t, it_type_t, col_t, e_src_t


def rgcn_gather_items_table(table, g, weight, type_shift, addend_table, drop_p, seed, relu, out, table16=None,
                            w16=None):
    """renet_rgcn_gather_items_table: the first RGCN layer reading source rows and the self-loop addend through
    g.node_ent from [N_ent, D] tables (forward, full graph).  table16 + w16 (gather_weight_bf16): source rows and
    relation blocks are read from the bf16 copies (the addend table stays fp32)."""
    d = table.shape[1]
    n_rows = out.shape[0]
    it_src_t, it_type_t, col_t, _ = g.table_items()
    b16 = table16 is not None and w16 is not None
    t0 = _timed()
    items = (table.shape[0], d) + _item_args(it_src_t, it_type_t, g, g.n_groups, col_t) + (_i32(g.node_ent), _f32(g.norm))
    tail = (weight.shape[0], int(type_shift), _f32(addend_table), float(drop_p), int(seed), int(relu), _f32(out),
            n_rows) + _heavy(g.heavy_rows) + (_stream(),)
    if b16:
        _check(lib().renet_rgcn_gather_items_table_bf16(table16.p.data_ptr(), table16.p.shape[1], *items,
                                                        w16.p.data_ptr(), w16.p.shape[1], *tail),
               'rgcn_gather_items_table_bf16')
    else:
        _check(lib().renet_rgcn_gather_items_table(_f32(table), *items, _f32(weight), *tail), 'rgcn_gather_items_table')
    eb = 2 if b16 else 4       # SURVEY 8d's ALGORITHMIC bytes: one source row per edge, one output (+ addend) row per node
    _gather_timed_end(t0, 'rgcn_gather_fwd_full', g.E, n_rows, d, weight, addend_table is not None, eb, eb)
    return out


def rgcn_bwd_prep(g_out, out, norm, relu, drop_p, seed, gn, g_loop):
    n, d = g_out.shape
    args = (_f32(g_out), _f32(out), _f32(norm), int(relu), float(drop_p), int(seed), n, d, _f32(gn), _f32(g_loop))
    if _fused_bounds(g_loop):                    # g_loop's operand bound comes out of the kernel that writes it
        _call_with_bounds('rgcn_bwd_prep_bounds', args, n * (d // 4), (g_loop,))
        return
    _check(lib().renet_rgcn_bwd_prep(*args, _stream()), 'rgcn_bwd_prep')


def rgcn_bwd_w(x, gn, e_src, e_dst, chunk_ptr, chunk_type, n_chunks, type_chunk_ptr, num_types, type_shift,
               dW, beta=0.0):
    d = x.shape[1]
    # feature tensors of 2 GiB and more: the entry with 64-bit addressing (as rgcn_gather_items falls back to the CSR
    # kernel); RENET_BWDW_64=1 forces it (tests)
    big = max(x.numel(), gn.numel()) * 4 >= (1 << 31) or os.environ.get('RENET_BWDW_64') == '1'
    nbytes = lib().renet_rgcn_bwd_w_workspace(n_chunks, d)
    ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
    t0 = _timed()
    fn = lib().renet_rgcn_bwd_w64 if big else lib().renet_rgcn_bwd_w
    _check(fn(_f32(x), _f32(gn), _i32(e_src), _i32(e_dst), _i32(chunk_ptr), _i32(chunk_type), n_chunks,
              _i32(type_chunk_ptr), num_types, type_shift, d, _f32(dW), float(beta), ws.data_ptr(), nbytes, _stream()),
           'rgcn_bwd_w')
    # SURVEY 8d backward-W: E * 2 rows + indices, dW written once
    _timed_end(t0, 'rgcn_bwd_w', nbytes=float(e_src.numel() * (2 * d * 4 + 8) + dW.numel() * 4))
    return dW


def _ld(t):
    if t.dim() != 2 or t.stride(1) != 1:
        raise RenetHipError('GEMM operands must be 2-D with unit inner stride')
    return t.stride(0)


def gemm_split_plan(ta, tb, m, n, k, lda=None, ldb=None, split_k=1, a_ptr=0, b_ptr=0):
    """What renet_gemm_f32_split would launch for this problem (host logic only, no GPU needed): dict with `kernel`
    ('fused' | 'two_phase_128' | 'two_phase_256' | 'weight_resident'), `raw` (raw-buffer loader), `xcd_order` (0 = plain
    tile order, w = XCD-aware order with panels of <= w tiles), `grid`, `split_k`."""
    lda = (m if ta else k) if lda is None else lda
    ldb = (k if tb else n) if ldb is None else ldb
    out = (ctypes.c_int * 8)()
    _check(lib().renet_gemm_split_plan(int(ta), int(tb), m, n, k, a_ptr, lda, b_ptr, ldb, split_k,
                                       ctypes.cast(out, ctypes.c_void_p)), 'renet_gemm_split_plan')
    names = {0: 'fused', 1: 'two_phase_128', 2: 'two_phase_256', 3: 'weight_resident', 4: 'bf16'}
    return {'kernel': names[out[0]], 'raw': bool(out[1]), 'xcd_order': out[2], 'grid': (out[3], out[4], out[5]),
            'split_k': out[6]}


def auto_split_k(m, n, k):
    """Deterministic split-K factor for outputs with too few 128x128 tiles to fill the chip (weight-gradient and
    dX-of-the-head shapes), from a small cost model in units of one k-tile step of a workgroup (~1.5 us):
        T(s) = rounds(tiles * s / 512 slots) * (ktiles / s + 6 [prologue + C store]) + s * M*N * 2.7e-6 [partial
        sums written and re-read by the reduce kernel]
    It reproduces the factors swept on MI355X (tools/gemm_sweep.py: dfeat 40 tiles -> 12 slices, dW_ih 35 -> 14,
    dW_loop 4 -> 128) and, unlike a pure fill heuristic, still splits a single-tile output (n_hidden = 100:
    100x100xK=46k would otherwise run 1440 k-tiles in ONE workgroup)."""
    return _split_k_model(m, n, k, tile_m=128, slots=512, full=256, smax=128)


def _split_k_model(m, n, k, tile_m, slots, full, smax):
    """auto_split_k's cost model on a grid of tile_m x 128 tiles with `slots` workgroups per round: no split from `full` tiles
    on, at most `smax` slices."""
    tiles = ((m + tile_m - 1) // tile_m) * ((n + 127) // 128)
    ktiles = (k + 31) // 32
    if tiles >= full or ktiles < 8:
        return 1
    per_slice = m * n * 2.7e-6
    best, best_t = 1, None
    for s in range(1, max(1, min(smax, ktiles // 4)) + 1):
        rounds = (tiles * s + slots - 1) // slots
        t = rounds * (ktiles / float(s) + 6.0) + (per_slice * s if s > 1 else 0.0)
        if best_t is None or t < best_t - 1e-9:
            best, best_t = s, t
    return best


def _gemm_front(what, m, n, k, k2, out, beta, split_k, device, n_out=None, planes=False):
    """What gemm, gemm_bf16s and gemm_planes do before their library call, for the [m, n] = [m, k] @ [k2, n] product whose
    `out` has n_out (default n) columns; planes: gemm_planes' grid -> (out, split_k, split-K workspace or None, its bytes)."""
    if k != k2:
        raise RenetHipError('%s inner dimensions differ: %d vs %d' % (what, k, k2))
    if out is None:
        if beta != 0.0:
            raise RenetHipError('beta != 0 needs an output tensor')
        out = torch.empty(m, n if n_out is None else n_out, device=device, dtype=torch.float32)
    if split_k is None:
        split_k = (auto_split_k_planes if planes else auto_split_k)(m, n, k)
    ws, ws_bytes = None, 0
    if split_k > 1:
        ws_bytes = lib().renet_gemm_workspace(m, n, split_k)
        ws = torch.empty(ws_bytes // 4, device=device, dtype=torch.float32)
    return out, split_k, ws, ws_bytes


def _gemm_timed_end(t0, ta, tb, m, n, k, split_k):
    if t0 is not None:
        _timed_end(t0, 'gemm_f32', flops=2.0 * m * n * k, tag=(int(ta), int(tb), m, n, k, split_k))


# 'bf16s'  : bf16 STORAGE: operands are (packed to) bf16 matrices in HBM, LDS-DMA staging, one bf16 MFMA product
#            (gemm_bf16s; BASELINE config 5 -- bench.py --dtype bf16)
# 'bf16'   : operands rounded to bf16 on the way into LDS, ONE v_mfma_f32_32x32x16_bf16 product, fp32 accumulate
#            (mixed precision for BASELINE config 5; tensors stay fp32 in memory)
# 'f32'    : v_mfma_f32_32x32x2_f32, exact fp32 products (gemm.hip)
# 'bf16x6' : fp32 operands split into 3 bf16 terms, 6 term products on v_mfma_f32_32x32x16_bf16 with fp32
#            accumulation (gemm_split.hip): fp32-class accuracy at 2.67x the matrix-pipe rate
# 'f16x3'  : fp32 operands, scaled per TENSOR by a power of two, split into 2 binary16 terms (22 significant bits),
#            3 term products on v_mfma_f32_32x32x16_f16 (gemm_h3.hip): GEMM errors within a small multiple of fp32's
#            own accumulation error (include/renet_hip.h), half the matrix instructions of bf16x6
# Default since round 4: 'bf16x6', the 24-bit split (fp32-class: every operand bit enters the product).  'f16x3' (22-bit
# operands, the round-3 default) is the opt-in FAST mode, 'f32' the exact-product mode; bench.py reports all three.
GEMM_MODE = os.environ.get('RENET_GEMM', 'bf16x6')

# Per-MODEL choice of the fp32-storage modes (round 4: the two split modes; round 5: 'f32' too): a model may carry
# `gemm_mode = 'f16x3' | 'bf16x6' | 'f32'` and its forward / backward passes then run inside `with gemm_mode(...)`; everything
# below reads the mode through current_mode() -- the GEMM entry point, and for 'f32' the exact GRU entries
# renet_gru_{fwd,bwd}_layouts_f32 (until round 4 the library chose them from RENET_GEMM alone).  GEMM_MODE stays the PROCESS
# default; 'bf16s' (operand STORAGE: packed weights, bf16 activations) remains process-wide: gemm_mode() accepts it only when
# it equals the process default.  (In a RENET_GEMM=f32 process the recurrences stay exact whatever a model asks for.)
_mode_override = threading.local()       # .mode: per THREAD (a prefetch / evaluation thread must not inherit another thread's
                                         # scope; ops._fwd_mode / _bwd_mode re-enter the scope on the autograd thread explicitly)
_PER_MODEL_MODES = ('bf16x6', 'f16x3', 'f32')


def current_mode():
    return getattr(_mode_override, 'mode', None) or GEMM_MODE


@contextlib.contextmanager
def gemm_mode(mode):
    """Scope in which the fp32-class GEMMs run in `mode` (None: no change)."""
    if mode is None or mode == current_mode():
        yield
        return
    if mode not in _PER_MODEL_MODES or GEMM_MODE not in _PER_MODEL_MODES:
        raise RenetHipError('gemm_mode(%r): only %s can be chosen per model, and only in a process whose default is one '
                            'of them (RENET_GEMM=%s)' % (mode, ' / '.join(_PER_MODEL_MODES), GEMM_MODE))
    old = getattr(_mode_override, 'mode', None)
    _mode_override.mode = mode
    try:
        yield
    finally:
        _mode_override.mode = old


class BF16Mat(object):
    """A matrix [R, C] stored as bf16 in a zero-padded [Rp, Cp] buffer (Rp, Cp multiples of 256): the operand format of
    gemm_bf16s (renet_pack_bf16 / a producer kernel that writes it directly)."""
    __slots__ = ('p', 'R', 'C')

    def __init__(self, p, R, C):
        self.p, self.R, self.C = p, R, C

    @property
    def shape(self):
        return (self.R, self.C)


def bf16_empty(r, c, device):
    """Uninitialised BF16Mat for a producer kernel that writes the bf16 format directly."""
    return BF16Mat(torch.empty((r + 255) & ~255, (c + 255) & ~255, device=device, dtype=torch.bfloat16), r, c)


def pack_bf16(x):
    """fp32 [R, C] (row-strided views allowed) -> BF16Mat."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise RenetHipError('pack_bf16 needs a 2-D float32 device tensor with unit inner stride')
    r, c = x.shape
    rp, cp = (r + 255) & ~255, (c + 255) & ~255
    p = torch.empty(rp, cp, device=x.device, dtype=torch.bfloat16)
    t0 = _timed()
    _check(lib().renet_pack_bf16(x.data_ptr(), r, c, x.stride(0), p.data_ptr(), _stream()), 'pack_bf16')
    _timed_end(t0, 'pack_bf16', nbytes=float(r * c * 4 + rp * cp * 2))
    return BF16Mat(p, r, c)


class _StreamGuard(object):
    """Orders consumers on OTHER streams behind the launch that filled a cached device buffer (the first
    bound request after an optimizer step may come from ops._Side's side stream; a main-stream GEMM that then hits
    the cache must not read the partial maxima before that launch has run).  Created right behind the producing
    launch on the producing stream; wait() is free on that same stream."""
    __slots__ = ('stream', 'event')

    def __init__(self, device):
        self.stream = torch.cuda.current_stream(device)
        self.event = torch.cuda.Event()
        self.event.record(self.stream)

    def wait(self, device):
        cur = torch.cuda.current_stream(device)
        if cur != self.stream:
            cur.wait_event(self.event)


# What is derived from a WEIGHT is cached between optimizer steps: parallel.HipAdam registers its parameters (stable
# addresses inside the flat buffer) and bumps the epoch after every update; any other tensor is packed / measured on every use.
class _Weight(object):
    """A registered weight: its shape, the tensor (weakly: its torch version counter is read) and the forms derived from it
    -- the bf16 copy (BF16Mat), the planes (PlanesMat), the partial maxima ((part, n)) -- each None or one entry
    (stamp, value, _StreamGuard or None) that holds while stamp == _weight_stamp(tensor)."""
    __slots__ = ('shape', 'ref', 'bf16', 'planes', 'maxima')

    def __init__(self):
        self.bf16 = self.planes = self.maxima = None


_weights = {}                  # data_ptr -> _Weight
_weight_epoch = [0]


def register_weights(tensors):
    for t in tensors:
        if t.dim() == 2 and t.is_contiguous():
            rec = _weights.setdefault(t.data_ptr(), _Weight())
            rec.shape, rec.ref = tuple(t.shape), weakref.ref(t)


def unregister_weights(tensors):
    for t in tensors:
        _weights.pop(t.data_ptr(), None)


def weights_changed():
    _weight_epoch[0] += 1


def _weight_stamp(t):
    return (_weight_epoch[0], t._version)           # in-place torch writes (load_state_dict) bump _version


def _registered(x, whole=False):
    """The record of the registered weight that tensor x is or is a leading row / column block of (W_ih[:, :live]), else
    None.  whole=True: only the weight itself counts."""
    rec = _weights.get(x.data_ptr())
    if rec is None or x.dim() != 2:
        return None
    if whole:
        return rec if tuple(x.shape) == rec.shape and x.is_contiguous() else None
    rows, cols = rec.shape
    return rec if x.stride(1) == 1 and x.stride(0) == cols and x.shape[0] <= rows and x.shape[1] <= cols else None


def _whole(x, rec):
    """The registered matrix of which x is a leading block."""
    return torch.as_strided(x, rec.shape, (rec.shape[1], 1))


def _derived(rec, form, x, make, guarded=True):
    """The value of rec's derived form `form` for weight (block) x as it is now: make() when there is none or the weight
    changed since.  guarded: a consumer on another stream is ordered behind the launch that made it."""
    ent, stamp = getattr(rec, form), _weight_stamp(x)
    if ent is None or ent[0] != stamp:
        ent = (stamp, make(), _StreamGuard(x.device) if guarded else None)
        setattr(rec, form, ent)
    if ent[2] is not None:
        ent[2].wait(x.device)                       # (no-op on the stream that made it)
    return ent[1]


def _as_bf16(x):
    """Operand of gemm_bf16s for tensor / BF16Mat x -> (BF16Mat, rows, cols) of the LOGICAL matrix x."""
    if isinstance(x, BF16Mat):
        return x, x.R, x.C
    rec = _registered(x)
    if rec is not None:                             # one cached copy of the whole weight serves its leading blocks too
        return _derived(rec, 'bf16', x, lambda: pack_bf16(_whole(x, rec)), guarded=False), x.shape[0], x.shape[1]
    m = pack_bf16(x)
    return m, m.R, m.C


# ---- PLANES (round 6): operands of the bf16x6 GEMM stored ALREADY split into their three bf16 terms ----------------
# The entity score head's three GEMMs (logits, dfeat, dW: 2/3 of the step's GEMM flops) re-split every operand element
# once per output tile that reads it (csrc/gemm_split.hip); here a tensor is split ONCE, by the kernel that produces it
# (softmax_ce_planes: the CE gradient; HipAdam: the head weight; pack_planes: the features), and the GEMM
# (csrc/gemm_planes.hip) stages the planes by LDS-DMA with no conversion work in its k-loop.  Same arithmetic (three RNE terms,
# six products, fp32 accumulation) as the in-loop split.  RENET_PLANES=0 keeps the in-loop split everywhere.
PLANES = os.environ.get('RENET_PLANES', '1') != '0'
PLANES_MIN_CLASSES = int(os.environ.get('RENET_PLANES_MIN_CLASSES', '2048'))


class PlanesMat(object):
    """A matrix [R, C] as three bf16 planes in ONE tensor p [3, Rp, Cp] (Rp, Cp multiples of 256, zero padding).  The
    elements of a plane are NOT row-major: they are stored in the T16 tile format of csrc/gemm_planes.hip (16 x 16 tiles of 512
    bytes; csrc/common.h renet_t16_off, tools/p6_layout_sim.py) -- p's trailing two dimensions only size the buffer;
    planes_to_dense() gives the row-major view (tests)."""
    __slots__ = ('p', 'R', 'C')

    def __init__(self, p, R, C):
        self.p, self.R, self.C = p, R, C

    @property
    def shape(self):
        return (self.R, self.C)

    @property
    def plane(self):
        return self.p.shape[1] * self.p.shape[2]


def planes_to_dense(m):
    """-> float32 [3, Rp, Cp]: the planes of PlanesMat m in row-major order (undoes the T16 tiling; tests / debugging)."""
    rp, cp = m.p.shape[1], m.p.shape[2]
    dev = m.p.device
    r = torch.arange(rp, device=dev).view(-1, 1)
    c = torch.arange(cp, device=dev).view(1, -1)
    i, j, tc = r & 15, c & 15, c >> 4
    idx = ((r >> 4) * (cp // 16) + tc) * 256 + (i ^ ((tc & 1) << 2)) * 16 + ((j >> 3) ^ ((i >> 3) & 1)) * 8 + (j & 7)
    return m.p.reshape(3, -1)[:, idx.reshape(-1)].reshape(3, rp, cp).float()


def planes_empty(r, c, device, zero=False):
    """PlanesMat for a producer kernel; zero=True when the producer does not write the padding itself."""
    rp, cp = (r + 255) & ~255, (c + 255) & ~255
    mk = torch.zeros if zero else torch.empty
    return PlanesMat(mk(3, rp, cp, device=device, dtype=torch.bfloat16), r, c)


def pack_planes(x, ones_col=False):
    """fp32 [R, C] (row-strided views allowed) -> PlanesMat; ones_col: one more column, all ones (gemm_planes' col_out)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise RenetHipError('pack_planes needs a 2-D float32 device tensor with unit inner stride')
    r, c = x.shape
    m = planes_empty(r, c + (1 if ones_col else 0), x.device)
    t0 = _timed()
    _check(lib().renet_pack_planes(x.data_ptr(), r, c, x.stride(0), int(bool(ones_col)), m.p.data_ptr(), _stream()),
           'pack_planes')
    _timed_end(t0, 'pack_planes', nbytes=float(r * c * 4 + 3 * m.plane * 2))
    return m


def weight_planes(w):
    """Planes of a weight matrix: a registered weight (parallel.HipAdam) is packed once per optimizer step -- or not at
    all when the optimizer kernel wrote them (note_weight_planes) -- anything else on every call."""
    rec = _registered(w, whole=True)
    return _derived(rec, 'planes', w, lambda: pack_planes(w)) if rec is not None else pack_planes(w)


def weight_planes_or_buffer(w):
    """For a consumer that can pack for itself (the C launch list, step_plan): (planes, stale) of a registered weight, or None
    for any other tensor.  stale = the cache holds nothing for the weight as it is now: `planes` is then an UNWRITTEN buffer,
    and the consumer reports it with note_weight_planes(w, planes) once its pack is enqueued."""
    rec = _registered(w, whole=True)
    if rec is None:
        return None
    ent = rec.planes
    if ent is not None and ent[0] == _weight_stamp(w):
        if ent[2] is not None:
            ent[2].wait(w.device)
        return ent[1], False
    return planes_empty(w.shape[0], w.shape[1], w.device), True


def note_weight_planes(w, mat):
    """The optimizer kernel has just written `mat` = the planes of the UPDATED weight w (call after weights_changed())."""
    rec = _registered(w, whole=True)
    if rec is not None:
        rec.planes = (_weight_stamp(w), mat, _StreamGuard(w.device))


def use_planes(weight, n_classes):
    """Whether a score head with this weight runs its GEMMs on planes: default fp32-class mode, a wide class dimension."""
    return (PLANES and current_mode() == 'bf16x6' and weight.is_cuda and n_classes >= PLANES_MIN_CLASSES and
            weight.dim() == 2 and weight.is_contiguous())


def auto_split_k_planes(m, n, k):
    """Split-K factor of gemm_planes (256 x 128 tiles, one workgroup per CU): auto_split_k's cost model on that grid."""
    return _split_k_model(m, n, k, tile_m=256, slots=256, full=128, smax=64)


def gemm_planes(a, b, ta=False, tb=False, out=None, bias=None, alpha=1.0, alpha_dev=None, beta=0.0, col_out=None,
                split_k=None):
    """out = alpha * alpha_dev * op(a) @ op(b) + bias + beta * out on PlanesMat operands (renet_gemm_planes).
    ta: a is stored [K, M]; tb: b is stored [N, K] (the conventions of gemm()).  col_out [M]: b's LAST column (a ones
    column, pack_planes(ones_col=True)) is not part of `out`; its product -- sum_k op(a)[m, k] -- goes to col_out."""
    if not (isinstance(a, PlanesMat) and isinstance(b, PlanesMat)):
        raise RenetHipError('gemm_planes needs PlanesMat operands')
    m, k = (a.C, a.R) if ta else (a.R, a.C)
    n, k2 = (b.R, b.C) if tb else (b.C, b.R)
    n_main = n - 1 if col_out is not None else n
    out, split_k, ws, ws_bytes = _gemm_front('gemm_planes', m, n, k, k2, out, beta, split_k, a.p.device, n_out=n_main,
                                             planes=True)
    if tuple(out.shape) != (m, n_main):
        raise RenetHipError('gemm_planes: output shape %r, expected %r' % (tuple(out.shape), (m, n_main)))
    if col_out is not None and (col_out.numel() != m or not col_out.is_contiguous()):
        raise RenetHipError('gemm_planes: col_out must be a contiguous vector of M floats')
    t0 = _timed()
    _check(lib().renet_gemm_planes(int(ta), int(not tb), m, n, k, float(alpha), _f32(alpha_dev), a.p.data_ptr(),
                                   a.p.shape[2], a.plane, b.p.data_ptr(), b.p.shape[2], b.plane, float(beta),
                                   out.data_ptr(), _ld(out), _f32(bias), _f32(col_out), split_k, _f32(ws), ws_bytes,
                                   _stream()), 'gemm_planes')
    _gemm_timed_end(t0, ta, tb, m, n_main, k, split_k)
    return out


def softmax_ce_planes(logits, target, grad_scale, row_loss=None):
    """-> (row_loss[B], PlanesMat (softmax - onehot) * grad_scale); the fp32 logits (row-strided view allowed) are not
    modified."""
    b, c = logits.shape
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    dl = planes_empty(b, c, logits.device)
    _check(lib().renet_softmax_ce_planes(logits.data_ptr(), _i32(target), b, c, _ld(logits), float(grad_scale),
                                         _f32(row_loss), dl.p.data_ptr(), dl.plane, dl.p.shape[2], dl.p.shape[1],
                                         _stream()), 'softmax_ce_planes')
    return row_loss, dl


def _copy_rows(a_row, q_row, b, what):
    for v, name in ((a_row, 'a_row'), (q_row, 'q_row')):
        if not (torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == b):
            raise RenetHipError('%s: %s must be a contiguous float32 device tensor with one entry per row' % (what, name))
    return a_row.data_ptr(), q_row.data_ptr()


def mix_ce_planes(logits, target, a_row, q_row, grad_scale, row_loss=None, want_da=True):
    """softmax_ce_planes for the loss through the copy mix (renet_mix_ce_planes): per row the gate a_row and the prior's mass
    on the gold column q_row (fp32 device [B]; a_row already zeroed where the prior abstains).  -> (row_loss[B] = -log((1 - a)
    p_gold + a q), PlanesMat (softmax - onehot) * grad_scale * s, d_a[B] = grad_scale * dL/da or None)."""
    b, c = logits.shape
    pa, pq = _copy_rows(a_row, q_row, b, 'mix_ce_planes')
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    d_a = torch.empty(b, device=logits.device, dtype=torch.float32) if want_da else None
    dl = planes_empty(b, c, logits.device)
    _check(lib().renet_mix_ce_planes(logits.data_ptr(), _i32(target), pa, pq, b, c, _ld(logits), float(grad_scale),
                                     _f32(row_loss), dl.p.data_ptr(), dl.plane, dl.p.shape[2], dl.p.shape[1], _f32(d_a),
                                     _stream()), 'mix_ce_planes')
    return row_loss, dl, d_a


def joint_mix_ce_planes(logits, target, a_row, q_row, lp_row, grad_scale, row_loss=None, want_da=True):
    """mix_ce_planes for the loss through the JOINT mix (renet_joint_mix_ce_planes): lp_row (fp32 device [B], <= 0) is the log-
    probability the relation head gives its gold class and q_row the prior's mass on the gold PAIR (joint_gold_rows).  ->
    (row_loss[B] = -log((1 - a) p_gold exp(lp) + a q), PlanesMat (softmax - onehot) * grad_scale * s, d_a[B] or None, s_row[B])."""
    b, c = logits.shape
    pa, pq = _copy_rows(a_row, q_row, b, 'joint_mix_ce_planes')
    plp = _lp_row(lp_row, b, 'joint_mix_ce_planes')
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    d_a = torch.empty(b, device=logits.device, dtype=torch.float32) if want_da else None
    s_row = torch.empty(b, device=logits.device, dtype=torch.float32)
    dl = planes_empty(b, c, logits.device)
    _check(lib().renet_joint_mix_ce_planes(logits.data_ptr(), _i32(target), pa, pq, plp, b, c, _ld(logits), float(grad_scale),
                                           _f32(row_loss), dl.p.data_ptr(), dl.plane, dl.p.shape[2], dl.p.shape[1], _f32(d_a),
                                           s_row.data_ptr(), _stream()), 'joint_mix_ce_planes')
    return row_loss, dl, d_a, s_row


def _lp_row(lp_row, b, what):
    if lp_row is None:
        raise RenetHipError('%s: lp_row is missing' % what)
    if not (torch.is_tensor(lp_row) and lp_row.is_cuda and lp_row.dtype == torch.float32 and lp_row.is_contiguous()
            and lp_row.numel() == b):
        raise RenetHipError('%s: lp_row must be a contiguous float32 device tensor with one entry per row' % what)
    return lp_row.data_ptr()


class F32Op(object):
    """An fp32 GEMM operand together with the bound on its largest magnitude that the f16x3 GEMM scales it by:
    `part` holds n <= 256 device floats whose maximum bounds max |t| (renet_maxabs_partials, or a known bound)."""
    __slots__ = ('t', 'part', 'n')

    def __init__(self, t, part=None, n=0):
        self.t, self.part, self.n = t, part, n

    @property
    def shape(self):
        return self.t.shape

    def bound(self):
        """(part, n), measured on first use: GEMMs that go to the weight-resident kernel never ask."""
        if self.part is None:
            self.part, self.n = _weight_or_measured_max(self.t)
        return self.part, self.n


def is_handle(x):
    """x is an operand handle made by operand() (to be kept for the GEMMs of the backward pass), not a plain tensor."""
    return isinstance(x, (BF16Mat, F32Op, PlanesMat))


def maxabs_partials(x):
    """-> (part, n): n <= 256 partial maxima of |x| for a 2-D fp32 matrix (row-strided views allowed)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise RenetHipError('maxabs_partials needs a 2-D float32 device tensor with unit inner stride')
    rows, cols = x.shape
    n = lib().renet_maxabs_blocks(rows, cols, _ld(x))
    part = torch.empty(n, device=x.device, dtype=torch.float32)
    t0 = _timed()
    _check(lib().renet_maxabs_partials(x.data_ptr(), rows, cols, _ld(x), part.data_ptr(), _stream()),
           'maxabs_partials')
    _timed_end(t0, 'maxabs', nbytes=float(rows * cols * 4))
    return part, n


_weight_jobs = {'key': None, 'table': None, 'parts': {}}     # one multi-array launch for all registered weights


def _measure_all_weights(device):
    """Measures the maxima of EVERY registered weight that is alive, contiguous, 16-byte aligned and a multiple of 4 elements
    long with one launch (renet_maxabs_partials_multi)."""
    live = {p: rec.ref() for p, rec in _weights.items()}
    ptrs = sorted(p for p, t in live.items() if t is not None and t.is_cuda and t.device == device
                  and t.numel() % 4 == 0 and p % 16 == 0 and t.data_ptr() == p)
    key = (tuple(ptrs), str(device))
    if _weight_jobs['key'] != key:
        rows, parts = [], {}
        for p in ptrs:
            shp = _weights[p].shape
            nb = lib().renet_maxabs_blocks(shp[0], shp[1], shp[1])
            part = torch.empty(nb, device=device, dtype=torch.float32)
            parts[p] = (part, nb)
            rows.append([p, shp[0] * shp[1] // 4, part.data_ptr(), nb])        # {x, n4, part, nblocks | pad}
        _weight_jobs.update(key=key, parts=parts,
                            table=torch.tensor(rows, dtype=torch.int64).to(device) if rows else None)
    if _weight_jobs['table'] is None:
        return
    t0 = _timed()
    _check(lib().renet_maxabs_partials_multi(_weight_jobs['table'].data_ptr(), len(ptrs), _stream()),
           'maxabs_partials_multi')
    if t0 is not None:
        _timed_end(t0, 'maxabs', nbytes=float(sum(_weights[p].shape[0] * _weights[p].shape[1] * 4 for p in ptrs)))
    guard = _StreamGuard(device)
    for p, bound in _weight_jobs['parts'].items():
        _weights[p].maxima = (_weight_stamp(live[p]), bound, guard)


def prefetch_weight_bounds(device):
    """Measure every registered weight NOW, on the current stream (parallel.HipAdam.step calls this right behind the
    update, on the stream the step runs on): the f16x3 GEMMs of the next step then only ever hit the cache."""
    if current_mode() == 'f16x3' and _weights:
        _measure_all_weights(device)


def _weight_or_measured_max(x):
    """A registered weight's maxima are cached until the next optimizer step (a leading row / column block of the
    weight is bounded by the whole weight's); anything else is measured."""
    rec = _registered(x)
    if rec is None:
        return maxabs_partials(x)
    if rec.maxima is None or rec.maxima[0][0] != _weight_epoch[0]:
        # first request after an optimizer step: every registered weight changed -- ONE launch measures them all
        _measure_all_weights(x.device)
    # (not coverable by the joint launch, or modified since: on its own)
    return _derived(rec, 'maxima', x, lambda: maxabs_partials(_whole(x, rec)))


def _f32op(x, bound=None):
    """F32Op of tensor x.  bound: a 1-element device tensor known to bound max |x| (else measured lazily)."""
    if isinstance(x, F32Op):
        return x
    return F32Op(x, bound, 1) if bound is not None else F32Op(x)


_const_bounds = {}


def const_bound(value, device):
    """1-element device tensor holding a known bound (GRU states: 1)."""
    key = (float(value), str(device))
    ent = _const_bounds.get(key)
    if ent is None:
        t = torch.full((1,), float(value), device=device, dtype=torch.float32)
        ent = (t, _StreamGuard(device) if t.is_cuda else None)
        _const_bounds[key] = ent
    if ent[1] is not None:
        ent[1].wait(device)                         # filled on another stream (ops._Side): order this one behind it
    return ent[0]


def operand_like(x, other):
    """Operand handle for x that reuses the magnitude bound of handle `other` (the caller knows |x| <= max |other|
    elementwise: the GRU's dGh against dGi); plain x outside f16x3 mode."""
    if current_mode() != 'f16x3' or not isinstance(other, F32Op):
        return operand(x)
    part, n = other.bound()
    return F32Op(x, part, n)


def _skinny_shape(ta, m, n, k, a, b, split_k):
    """Mirror of renet_gemm_skinny_eligible (gemm_skinny.hip): these shapes run the weight-resident bf16x6 kernel in
    every fp32-class mode and need no magnitude bounds."""
    return (not ta and split_k == 1 and n <= 256 and 16 <= k <= 208 and k % 4 == 0 and m >= 256 and
            a.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and
            os.environ.get('RENET_GEMM_SKINNY', '1') != '0')


# Operand bounds emitted by the kernel that WROTE the tensor (seq_assemble_fwd, concat3_fwd, rgcn_bwd_prep in f16x3
# mode) ride on the tensor OBJECT (`_renet_bound` = (part, n)) and are picked up by operand() instead of a
# renet_maxabs_partials pass; a tensor that arrives without the attribute (re-wrapped by autograd, a view, a copy) is
# simply measured.  The producers' outputs are never modified in place.  RENET_FUSED_BOUNDS=0 turns this off.
def _fused_bounds(t):
    return current_mode() == 'f16x3' and t.is_cuda and t.numel() > 0 and os.environ.get('RENET_FUSED_BOUNDS', '1') != '0'


def _note_bound(t, part, n):
    t._renet_bound = (part, n)


def _call_with_bounds(entry, args, elems, outs):
    """The `_bounds` variant of a producer kernel: renet_<entry>(*args, one block of partial maxima per tensor of `outs`,
    stream), the blocks sized for `elems` units of work and noted on the tensors they bound."""
    nparts = lib().renet_bound_parts(elems)
    parts = torch.empty(len(outs), nparts, device=outs[0].device, dtype=torch.float32)
    _check(getattr(lib(), 'renet_' + entry)(*args, *[p.data_ptr() for p in parts], _stream()), entry)
    for t, p in zip(outs, parts):
        _note_bound(t, p, nparts)


_lazy_shells = {}          # (data_ptr, shape) of an uninitialised fp32 shell -> the BF16Mat it stands for


def lazy_shell(mat, device):
    """fp32 tensor of mat's logical shape whose VALUES ARE NEVER WRITTEN: the autograd-visible stand-in of a tensor
    that exists only as a bf16 operand matrix (bf16-storage mode); operand() resolves it to `mat`."""
    x = torch.empty(mat.R, mat.C, device=device, dtype=torch.float32)
    x._renet_bf16 = mat
    key = (x.data_ptr(), (mat.R, mat.C))
    _lazy_shells[key] = mat
    # the address-keyed entry lives exactly as long as the shell OBJECT (a shell dropped before it reached
    # operand() must not leave an entry that a later fp32 tensor at the same address and shape would resolve to)
    weakref.finalize(x, _drop_lazy_shell, key, mat)
    return x


def _drop_lazy_shell(key, mat):
    if _lazy_shells.get(key) is mat:
        del _lazy_shells[key]


def operand(x, bound=None):
    """GEMM operand for activation tensor x: in bf16-storage mode its bf16 copy (packed ONCE, to be handed to every
    GEMM that consumes x), in f16x3 mode x with the bound on its magnitude (ONE pass over x, or `bound`: a 1-element
    device tensor the producer knows to bound max |x|), otherwise x itself."""
    if isinstance(x, (BF16Mat, F32Op)):
        return x
    lazy = getattr(x, '_renet_bf16', None)          # a producer already wrote the bf16 form (ops.SeqAssembleFn)
    if lazy is None:
        # the attribute rides on the Python object; should autograd ever hand over a re-wrapped tensor, the shell is
        # still recognised by its storage -- an uninitialised shell must never be packed
        lazy = _lazy_shells.pop((x.data_ptr(), tuple(x.shape)), None)
    else:
        _lazy_shells.pop((x.data_ptr(), tuple(x.shape)), None)
    if lazy is not None:
        return lazy
    if current_mode() == 'bf16s':
        return pack_bf16(x)
    if current_mode() == 'f16x3' and x.is_cuda and x.dim() == 2:
        noted = getattr(x, '_renet_bound', None)
        if noted is not None and bound is None:
            return F32Op(x, noted[0], noted[1])
        return _f32op(x, bound)
    return x


def gemm_bf16s(a, b, ta=False, tb=False, out=None, bias=None, alpha=1.0, beta=0.0, split_k=None):
    """gemm() on bf16-STORED operands (fp32 tensors are packed first; registered weights come from the cache).
    A leading block of a cached matrix along the CONTRACTION dimension is only valid when the block ends on a 64-wide
    k stage (or at the matrix edge, where the padding is zero) -- otherwise it is packed afresh."""
    def prep(x, k_axis):
        m, r, c = _as_bf16(x)
        klen, kfull = (r, m.R) if k_axis == 0 else (c, m.C)
        if klen != kfull and (klen % 64) != 0:
            m = pack_bf16(x)
            r, c = m.R, m.C
        return m, r, c
    pa, ar, ac = prep(a, 0 if ta else 1)
    pb, br, bc = prep(b, 1 if tb else 0)
    m, k = (ac, ar) if ta else (ar, ac)
    n, k2 = (br, bc) if tb else (bc, br)
    out, split_k, ws, ws_bytes = _gemm_front('gemm', m, n, k, k2, out, beta, split_k, pa.p.device)
    t0 = _timed()
    _check(lib().renet_gemm_bf16s(int(ta), int(not tb), m, n, k, float(alpha), pa.p.data_ptr(), pa.p.shape[1],
                                  pb.p.data_ptr(), pb.p.shape[1], float(beta), out.data_ptr(), _ld(out), _f32(bias),
                                  split_k, _f32(ws), ws_bytes, _stream()), 'gemm_bf16s')
    _gemm_timed_end(t0, ta, tb, m, n, k, split_k)
    return out


def gemm(a, b, ta=False, tb=False, out=None, bias=None, alpha=1.0, beta=0.0, split_k=None, mode=None):
    """out = alpha * op(a) @ op(b) + bias + beta * out.  a/b may be row-strided views.
    split_k=None picks the deterministic split-K factor automatically."""
    if (mode or current_mode()) == 'bf16s' or isinstance(a, BF16Mat) or isinstance(b, BF16Mat):
        return gemm_bf16s(a, b, ta=ta, tb=tb, out=out, bias=bias, alpha=alpha, beta=beta, split_k=split_k)
    md = mode or current_mode()
    opa, opb = a, b
    if isinstance(a, F32Op):
        a = a.t
    if isinstance(b, F32Op):
        b = b.t
    if not (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32):
        raise RenetHipError('gemm operands must be float32 device tensors')
    m, k = (a.shape[1], a.shape[0]) if ta else (a.shape[0], a.shape[1])
    k2, n = (b.shape[1], b.shape[0]) if tb else (b.shape[0], b.shape[1])
    out, split_k, ws, ws_bytes = _gemm_front('gemm', m, n, k, k2, out, beta, split_k, a.device)
    if md == 'f16x3' and _skinny_shape(ta, m, n, k, a, b, split_k):
        md = 'bf16x6'
    if md == 'f16x3':
        (pa, na), (pb, nb) = _f32op(opa).bound(), _f32op(opb).bound()     # (measured outside the GEMM's timer)
    t0 = _timed()
    if md == 'f16x3':
        _check(lib().renet_gemm_f32_h3(int(ta), int(tb), m, n, k, float(alpha), a.data_ptr(), _ld(a), b.data_ptr(),
                                       _ld(b), float(beta), out.data_ptr(), _ld(out), _f32(bias), split_k, _f32(ws),
                                       ws_bytes, pa.data_ptr(), na, pb.data_ptr(), nb, _stream()),
               'gemm_f32_h3')
    else:
        fn = lib().renet_gemm_f32_split if md == 'bf16x6' else lib().renet_gemm_bf16 if md == 'bf16' else \
            lib().renet_gemm_f32
        _check(fn(int(ta), int(tb), m, n, k, float(alpha), a.data_ptr(), _ld(a), b.data_ptr(),
                  _ld(b), float(beta), out.data_ptr(), _ld(out), _f32(bias), split_k, _f32(ws),
                  ws_bytes, _stream()), 'gemm_f32')
    _gemm_timed_end(t0, ta, tb, m, n, k, split_k)
    return out


def colsum(x, out=None, beta=0.0):
    """out = beta * out + column sums of x (fp32 tensor or BF16Mat)."""
    fn, what, t = (lib().renet_colsum_bf16, 'colsum_bf16', x.p) if isinstance(x, BF16Mat) else \
        (lib().renet_colsum, 'colsum', x)
    m, n = x.shape
    if out is None:
        if beta != 0.0:
            raise RenetHipError('beta != 0 needs an output tensor')
        out = torch.empty(n, device=t.device, dtype=torch.float32)
    nbytes = lib().renet_colsum_workspace(m, n)
    ws = torch.empty(nbytes // 4, device=t.device, dtype=torch.float32) if nbytes else None
    _check(fn(t.data_ptr(), m, n, _ld(t), _f32(out), float(beta), _f32(ws), nbytes, _stream()), what)
    return out


def scale_by_device_scalar(x, g, bound_in=None):
    """x *= g in place, g a 0-dim / 1-element DEVICE tensor (no host sync; g == 1 leaves x untouched).
    bound_in: a host float bounding max |x| before the scaling -> returns the 1-element device tensor |g| * bound_in
    (fp32 tensors only), the operand bound of the f16x3 GEMMs that consume x; otherwise returns x."""
    if bound_in is not None and not isinstance(x, BF16Mat):
        if not x.is_contiguous():
            raise RenetHipError('scale_by_device_scalar needs a contiguous tensor')
        out = torch.empty(1, device=x.device, dtype=torch.float32)
        _check(lib().renet_scale_by_device_scalar_bound(_f32(x), x.numel(), _f32(g), float(bound_in), out.data_ptr(),
                                                        _stream()), 'scale_by_device_scalar_bound')
        return out
    if isinstance(x, BF16Mat):
        _check(lib().renet_scale_bf16_by_device_scalar(x.p.data_ptr(), x.p.numel(), _f32(g), _stream()),
               'scale_bf16_by_device_scalar')
        return x
    if not x.is_contiguous():
        raise RenetHipError('scale_by_device_scalar needs a contiguous tensor')
    _check(lib().renet_scale_by_device_scalar(_f32(x), x.numel(), _f32(g), _stream()), 'scale_by_device_scalar')
    return x


def seq_assemble_fwd(h2, ent, rel, glob, subj_row, row_ent, row_rel, glob_row, drop_p, seed_x, seed_xr):
    s, d = subj_row.numel(), h2.shape[1]
    x = torch.empty(s, 4 * d, device=h2.device, dtype=torch.float32)
    xr = torch.empty(s, 3 * d, device=h2.device, dtype=torch.float32)
    args = (_f32(h2), _f32(ent), _f32(rel), _f32(glob), _i32(subj_row), _i32(row_ent), _i32(row_rel), _i32(glob_row), s, d,
            float(drop_p), int(seed_x), int(seed_xr), _f32(x), _f32(xr))
    if _fused_bounds(x):                         # the operand bounds of X / Xr come out of the kernel that writes them
        _call_with_bounds('seq_assemble_fwd_bounds', args, s * d, (x, xr))
    else:
        _check(lib().renet_seq_assemble_fwd(*args, _stream()), 'seq_assemble_fwd')
    return x, xr


def seq_assemble_fwd_bf16(h2, ent, rel, glob, subj_row, row_ent, row_rel, glob_row, drop_p, seed_x, seed_xr):
    """seq_assemble_fwd with X / Xr written as bf16 operand matrices (-> BF16Mat, BF16Mat); no fp32 copy exists."""
    s, d = subj_row.numel(), h2.shape[1]
    x, xr = bf16_empty(s, 4 * d, h2.device), bf16_empty(s, 3 * d, h2.device)
    _check(lib().renet_seq_assemble_fwd_bf16(_f32(h2), _f32(ent), _f32(rel), _f32(glob), _i32(subj_row), _i32(row_ent),
                                             _i32(row_rel), _i32(glob_row), s, d, float(drop_p), int(seed_x),
                                             int(seed_xr), x.p.data_ptr(), x.p.shape[1], xr.p.data_ptr(),
                                             xr.p.shape[1], x.p.shape[0], _stream()), 'seq_assemble_fwd_bf16')
    return x, xr


def softmax_ce_bf16(logits, target, grad_scale, row_loss=None):
    """-> (row_loss[B], BF16Mat (softmax - onehot) * grad_scale); the fp32 logits are not modified."""
    b, c = logits.shape
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    dl = bf16_empty(b, c, logits.device)
    _check(lib().renet_softmax_ce_bf16(logits.data_ptr(), _i32(target), b, c, _ld(logits), float(grad_scale),
                                       _f32(row_loss), dl.p.data_ptr(), dl.p.shape[1], min((b + 63) & ~63, dl.p.shape[0]),
                                       _stream()), 'softmax_ce_bf16')
    return row_loss, dl


def seq_assemble_bwd(dx, dxr, step_off, num_steps, num_seq, d, drop_p, seed_x, seed_xr):
    """-> (dRows[S,D], dEntSeq[num_seq,D], dRelSeq[num_seq,D]); step_off: device int32 [L+1]."""
    s = dx.shape[0]
    d_rows = torch.empty(s, d, device=dx.device, dtype=torch.float32)
    d_ent = torch.empty(num_seq, d, device=dx.device, dtype=torch.float32)
    d_rel = torch.empty(num_seq, d, device=dx.device, dtype=torch.float32)
    _check(lib().renet_seq_assemble_bwd(_f32(dx), _f32(dxr), _i32(step_off), num_steps, s, num_seq, d,
                                        float(drop_p), int(seed_x), int(seed_xr), _f32(d_rows), _f32(d_ent),
                                        _f32(d_rel), _stream()), 'seq_assemble_bwd')
    return d_rows, d_ent, d_rel


def gru_fwd(gi, step_off_host, hdim, w_hh, b_hh, out_rows=0):
    """gi [S,3H] packed; step_off_host: ctypes int32 array (L+1).  Returns (h_last[max(B, out_rows), H] with
    rows >= B zero, saved[S,5H]).  (One-problem form of gru_fwd_layouts, which also selects the bf16-mode kernels.)"""
    hs, svs = gru_fwd_layouts([gi], [step_off_host], hdim, [w_hh], [b_hh], [out_rows])
    return hs[0], svs[0]


def gru_bwd(dh_last, step_off_host, hdim, w_hh, saved):
    d_gis, d_ghs = gru_bwd_layouts([dh_last], [step_off_host], hdim, [w_hh], [saved])
    return d_gis[0], d_ghs[0]


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _offs(step_offs):
    return ((ctypes.c_void_p * len(step_offs))(*[ctypes.cast(o, c_void_p).value for o in step_offs]),
            (ctypes.c_int * len(step_offs))(*[len(o) - 1 for o in step_offs]))


def _seqs(o):
    return (o[1] - o[0]) if len(o) > 1 else 0


_GRU_SUFFIX = {'bf16s': '_bf16', 'f32': '_f32'}          # current_mode() -> entry point suffix (any other mode: none)


def _gru_call(n, step_offs, hdim, operands):
    """What every recurrence call needs: checks the fp32 operands -> (bmax, workspace, its bytes, offset pointers, Ls)."""
    for t in operands:
        _f32(t)
    bmax = max([_seqs(o) for o in step_offs] + [0])
    nbytes = n * lib().renet_gru_workspace(int(bmax), hdim)
    ws = torch.empty(max(nbytes // 4, 1), device=operands[0].device, dtype=torch.float32)
    return (bmax, ws, nbytes) + _offs(step_offs)


def _gru_timed_end(t0, hdim, packed):
    """The library calls since t0 = _timed() as 'gru_recurrence': h_{t-1} @ W_hh^T (backward: d_gates @ W_hh) per step,
    2 * 3H * H flops per packed row of the tensors in `packed`."""
    if t0 is not None:
        _timed_end(t0, 'gru_recurrence', flops=sum(2.0 * 3 * hdim * hdim * t.shape[0] for t in packed))


def gru_fwd_multi(gis, step_off_host, hdim, w_hhs, b_hhs, out_rows=0):
    """n GRUs over the same packed layout in one launch -> ([h_last...], [saved...]); h_last has
    max(B, out_rows) rows, the ones past B zero."""
    L = len(step_off_host) - 1
    out_rows = max(int(out_rows), _seqs(step_off_host))
    dev = gis[0].device
    hs = [torch.empty(out_rows, hdim, device=dev, dtype=torch.float32) for _ in gis]
    svs = [torch.empty(g.shape[0], 5 * hdim, device=dev, dtype=torch.float32) for g in gis]
    _, ws, nbytes, _, _ = _gru_call(len(gis), [step_off_host], hdim, list(gis) + list(w_hhs) + list(b_hhs))
    t0 = _timed()
    _check(lib().renet_gru_fwd_multi(len(gis), _ptrs(gis), ctypes.cast(step_off_host, c_void_p), L, hdim,
                                     _ptrs(w_hhs), _ptrs(b_hhs), _ptrs(hs), out_rows, _ptrs(svs), ws.data_ptr(),
                                     nbytes, _stream()), 'gru_fwd_multi')
    _gru_timed_end(t0, hdim, gis)
    return hs, svs


def gru_bwd_multi(dh_lasts, step_off_host, hdim, w_hhs, saveds):
    L = len(step_off_host) - 1
    n = len(dh_lasts)
    dev = saveds[0].device
    d_gis = [torch.empty(s.shape[0], 3 * hdim, device=dev, dtype=torch.float32) for s in saveds]
    d_ghs = [torch.empty(s.shape[0], 3 * hdim, device=dev, dtype=torch.float32) for s in saveds]
    _, ws, nbytes, _, _ = _gru_call(n, [step_off_host], hdim, list(dh_lasts) + list(w_hhs) + list(saveds))
    t0 = _timed()
    _check(lib().renet_gru_bwd_multi(n, _ptrs(dh_lasts), ctypes.cast(step_off_host, c_void_p), L, hdim,
                                     _ptrs(w_hhs), _ptrs(saveds), _ptrs(d_gis), _ptrs(d_ghs), ws.data_ptr(),
                                     nbytes, _stream()), 'gru_bwd_multi')
    _gru_timed_end(t0, hdim, saveds)
    return d_gis, d_ghs


def gru_fwd_layouts(gis, step_offs, hdim, w_hhs, b_hhs, out_rows):
    """n <= 4 GRUs of up to two packed layouts in one launch (renet_gru_fwd_layouts): step_offs[k] is the host
    offset array of problem k (problems of one layout pass the SAME object), out_rows[k] its h_last height.
    -> ([h_last...], [saved...])."""
    n = len(gis)
    dev = gis[0].device
    rows = [max(int(r), _seqs(o)) for r, o in zip(out_rows, step_offs)]
    hs = [torch.empty(r, hdim, device=dev, dtype=torch.float32) for r in rows]
    svs = [torch.empty(g.shape[0], 5 * hdim, device=dev, dtype=torch.float32) for g in gis]
    _, ws, nbytes, so, ls = _gru_call(n, step_offs, hdim, list(gis) + list(w_hhs) + list(b_hhs))
    fn = getattr(lib(), 'renet_gru_fwd_layouts' + _GRU_SUFFIX.get(current_mode(), ''))
    t0 = _timed()
    _check(fn(n, _ptrs(gis), so, ls, hdim, _ptrs(w_hhs), _ptrs(b_hhs), _ptrs(hs), (ctypes.c_int * n)(*rows),
              _ptrs(svs), ws.data_ptr(), nbytes, _stream()), 'gru_fwd_layouts')
    _gru_timed_end(t0, hdim, gis)
    return hs, svs


def gru_bwd_layouts(dh_lasts, step_offs, hdim, w_hhs, saveds, out_bf16=False):
    """out_bf16 (bf16-storage mode only): d_gi / d_gh come back as BF16Mat operand matrices instead of fp32 tensors."""
    n = len(dh_lasts)
    dev = saveds[0].device
    if out_bf16:
        if current_mode() != 'bf16s':
            raise RenetHipError('bf16 GRU gradients exist in bf16-storage mode only')
        d_gis = [bf16_empty(s_.shape[0], 3 * hdim, dev) for s_ in saveds]
        d_ghs = [bf16_empty(s_.shape[0], 3 * hdim, dev) for s_ in saveds]
        lds = {m.p.shape[1] for m in d_gis + d_ghs}
        assert len(lds) == 1
        for m in d_gis + d_ghs:
            _check(lib().renet_bf16_zero_padding(m.p.data_ptr(), m.R, m.C, m.p.shape[1], m.p.shape[0], _stream()),
                   'bf16_zero_padding')
    else:
        d_gis = [torch.empty(s.shape[0], 3 * hdim, device=dev, dtype=torch.float32) for s in saveds]
        d_ghs = [torch.empty(s.shape[0], 3 * hdim, device=dev, dtype=torch.float32) for s in saveds]
    bmax, ws, nbytes, so, ls = _gru_call(n, step_offs, hdim, list(dh_lasts) + list(w_hhs) + list(saveds))
    head = (n, _ptrs(dh_lasts), so, ls, hdim, _ptrs(w_hhs), _ptrs(saveds))
    tail = (ws.data_ptr(), nbytes, _stream())
    t0 = _timed()
    rc = -2                                                  # RENET_ERR_UNSUPPORTED: not done by a special entry
    if out_bf16:
        rc = lib().renet_gru_bwd_layouts_bf16out(*head, _ptrs([m.p for m in d_gis]), _ptrs([m.p for m in d_ghs]),
                                                 lds.pop(), *tail)
        _check(rc, 'gru_bwd_layouts_bf16out')
    elif _fused_bounds(d_gis[0]) and bmax > 0:
        # the kernel that writes dGi also emits its operand bound (one max |dGi| per workgroup)
        nparts = lib().renet_gru_bound_parts(int(bmax))
        parts = torch.empty(n, nparts, device=dev, dtype=torch.float32)
        rc = lib().renet_gru_bwd_layouts_bounds(*head, _ptrs(d_gis), _ptrs(d_ghs),
                                                _ptrs([parts[k] for k in range(n)]), *tail)
        if rc == 0:
            for k in range(n):
                _note_bound(d_gis[k], parts[k], nparts)
        elif rc != -2:                                       # (-2: another recurrence is selected)
            _check(rc, 'gru_bwd_layouts_bounds')
    if rc == -2:
        fn = getattr(lib(), 'renet_gru_bwd_layouts' + _GRU_SUFFIX.get(current_mode(), ''))
        _check(fn(*head, _ptrs(d_gis), _ptrs(d_ghs), *tail), 'gru_bwd_layouts')
    _gru_timed_end(t0, hdim, saveds)
    return d_gis, d_ghs


def concat3_fwd(a, ia, hmid, c, ic, drop_p, seed):
    b, d = hmid.shape
    parts = 3 if c is not None else 2
    feat = torch.empty(b, parts * d, device=hmid.device, dtype=torch.float32)
    args = (_f32(a), _i32(ia), _f32(hmid), _f32(c), _i32(ic), b, d, float(drop_p), int(seed), _f32(feat))
    if _fused_bounds(feat):
        _call_with_bounds('concat3_fwd_bounds', args, b * parts * (d // 4), (feat,))
    else:
        _check(lib().renet_concat3_fwd(*args, _stream()), 'concat3_fwd')
    return feat


def concat3_bwd(dfeat, d, parts, drop_p, seed):
    b = dfeat.shape[0]
    da = torch.empty(b, d, device=dfeat.device, dtype=torch.float32)
    dh = torch.empty(b, d, device=dfeat.device, dtype=torch.float32)
    dc = torch.empty(b, d, device=dfeat.device, dtype=torch.float32) if parts == 3 else None
    _check(lib().renet_concat3_bwd(_f32(dfeat), b, d, parts, float(drop_p), int(seed), _f32(da), _f32(dh),
                                   _f32(dc), _stream()), 'concat3_bwd')
    return da, dh, dc


def dropout(x, drop_p, seed):
    y = torch.empty_like(x)
    _check(lib().renet_dropout(_f32(x), x.numel(), float(drop_p), int(seed), _f32(y), _stream()), 'dropout')
    return y


def softmax_ce(logits, target, grad_scale, want_grad, row_loss=None):
    """Returns row_loss[B] (written into `row_loss` when given); if want_grad, logits is OVERWRITTEN with
    (softmax - onehot) * grad_scale."""
    b, c = logits.shape
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    _check(lib().renet_softmax_ce(logits.data_ptr(), _i32(target), b, c, _ld(logits), float(grad_scale),
                                  _f32(row_loss), logits.data_ptr() if want_grad else None, _stream()),
           'softmax_ce')
    return row_loss


def mix_ce(logits, target, a_row, q_row, grad_scale, want_grad, row_loss=None, want_da=True):
    """softmax_ce for the loss through the copy mix (renet_mix_ce; a_row / q_row as for mix_ce_planes): -> (row_loss[B],
    d_a[B] or None); if want_grad, logits is OVERWRITTEN with (softmax - onehot) * grad_scale * s."""
    b, c = logits.shape
    pa, pq = _copy_rows(a_row, q_row, b, 'mix_ce')
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    d_a = torch.empty(b, device=logits.device, dtype=torch.float32) if want_da else None
    _check(lib().renet_mix_ce(logits.data_ptr(), _i32(target), pa, pq, b, c, _ld(logits), float(grad_scale),
                              _f32(row_loss), logits.data_ptr() if want_grad else None, _f32(d_a), _stream()), 'mix_ce')
    return row_loss, d_a


def joint_mix_ce(logits, target, a_row, q_row, lp_row, grad_scale, want_grad, row_loss=None, want_da=True):
    """mix_ce for the loss through the JOINT mix (renet_joint_mix_ce; lp_row as for joint_mix_ce_planes): -> (row_loss[B],
    d_a[B] or None, s_row[B]); if want_grad, logits is OVERWRITTEN with (softmax - onehot) * grad_scale * s."""
    b, c = logits.shape
    pa, pq = _copy_rows(a_row, q_row, b, 'joint_mix_ce')
    plp = _lp_row(lp_row, b, 'joint_mix_ce')
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    d_a = torch.empty(b, device=logits.device, dtype=torch.float32) if want_da else None
    s_row = torch.empty(b, device=logits.device, dtype=torch.float32)
    _check(lib().renet_joint_mix_ce(logits.data_ptr(), _i32(target), pa, pq, plp, b, c, _ld(logits), float(grad_scale),
                                    _f32(row_loss), logits.data_ptr() if want_grad else None, _f32(d_a), s_row.data_ptr(),
                                    _stream()), 'joint_mix_ce')
    return row_loss, d_a, s_row


def soft_ce_sparse(logits, tgt_ptr, tgt_col, tgt_w, grad_scale, want_grad, row_loss=None):
    """renet_soft_ce_sparse on logits [B, C] (fp32, unit inner stride) with the CSR soft targets tgt_ptr [B + 1] (int32),
    tgt_col [nnz] (int32; per row distinct, ascending) and tgt_w [nnz] (fp32, >= 0; a row need not sum to 1): returns
    row_loss[B] = W logsumexp(row) - sum_k w_k row[col_k] (written into `row_loss` when given); if want_grad, logits is
    OVERWRITTEN with grad_scale * (W softmax(row) - w)."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise RenetHipError('soft_ce_sparse needs a 2-D float32 device tensor')
    b, c = logits.shape
    if tgt_ptr.numel() != b + 1 or tgt_col.numel() != tgt_w.numel():
        raise RenetHipError('soft_ce_sparse: shape mismatch')
    if row_loss is None:
        row_loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    _check(lib().renet_soft_ce_sparse(logits.data_ptr(), b, c, _ld(logits), _i32(tgt_ptr), _i32(tgt_col), _f32(tgt_w),
                                      float(grad_scale), _f32(row_loss), logits.data_ptr() if want_grad else None,
                                      _stream()), 'soft_ce_sparse')
    return row_loss


def rank_rows(scores, label, filt_ptr=None, filt_col=None, filtered=True, want_loss=True):
    """renet_rank_rows on scores [n, C] (fp32, unit inner stride; not written) for the gold columns label [n] (int32):
    -> (counts, row_loss): counts is int32 [2, n] = (greater, equal) -- the rank with averaged ties is
    greater + (equal - 1) / 2 + 1 -- and row_loss [n] = logsumexp(row) - row[label] (None unless want_loss).
    filtered: compare sigmoid(score) and give the columns of the CSR lists filt_ptr [n + 1] / filt_col (int32; every column at
    most once per row) the value 0; filtered=False compares the scores themselves and takes no lists."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2):
        raise RenetHipError('rank_rows needs a 2-D float32 device tensor')
    n, c = scores.shape
    if label.numel() != n or (filt_ptr is not None and (filt_col is None or filt_ptr.numel() != n + 1)):
        raise RenetHipError('rank_rows: shape mismatch')
    counts = torch.empty(2, n, device=scores.device, dtype=torch.int32)
    row_loss = torch.empty(n, device=scores.device, dtype=torch.float32) if want_loss else None
    t0 = _timed()
    _check(lib().renet_rank_rows(scores.data_ptr(), max(_ld(scores), c) if n == 1 else _ld(scores), n, c, _i32(label),
                                 _i32(filt_ptr), _i32(filt_col), int(bool(filtered)), counts[0].data_ptr(),
                                 counts[1].data_ptr(), _f32(row_loss), _stream()), 'rank_rows')
    _timed_end(t0, 'rank_rows', nbytes=float(n * c * 4))
    return counts, row_loss


def rank_rows3(scores, label, cols_a, start_a, count_a, cols_t, start_t, count_t, want_loss=True):
    """renet_rank_rows3 on scores [n, C] (fp32, unit inner stride; not written) for the gold columns label [n] (int32):
    -> (counts, row_loss): counts is int32 [6, n] = raw (greater, equal), filtered (greater, equal), time_filtered (greater,
    equal) -- rank = greater + (equal - 1) / 2 + 1 each -- from ONE read of the scores; row_loss as rank_rows gives it.
    (cols_a, start_a [n], count_a [n]) is the time-agnostic filter list of every row as a range of the resident column
    table cols_a (filter_index.FilterIndex.ranges; int32), (cols_t, start_t, count_t) the time-aware one; a list given as
    three Nones (or an empty table) leaves that setting unfiltered: the sigmoid counts alone."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2):
        raise RenetHipError('rank_rows3 needs a 2-D float32 device tensor')
    n, c = scores.shape
    lists = []
    for cols, start, count in ((cols_a, start_a, count_a), (cols_t, start_t, count_t)):
        if cols is None and start is None and count is None:
            lists += [None, None, None, 0]
            continue
        if cols is None or start is None or count is None or start.numel() != n or count.numel() != n:
            raise RenetHipError('rank_rows3: a filter list is (cols, start [n], count [n])')
        # (an empty table has no storage to point at: no list)
        lists += [_i32(cols), _i32(start), _i32(count), cols.numel()] if cols.numel() else [None, None, None, 0]
    if label.numel() != n:
        raise RenetHipError('rank_rows3: shape mismatch')
    counts = torch.empty(6, n, device=scores.device, dtype=torch.int32)
    row_loss = torch.empty(n, device=scores.device, dtype=torch.float32) if want_loss else None
    t0 = _timed()
    _check(lib().renet_rank_rows3(scores.data_ptr(), max(_ld(scores), c) if n == 1 else _ld(scores), n, c, _i32(label),
                                  *lists, counts.data_ptr(), _f32(row_loss), _stream()), 'rank_rows3')
    _timed_end(t0, 'rank_rows3', nbytes=float(n * c * 4))
    return counts, row_loss


TOPK_ROWS_MAX_C = 32768                 # renet_topk_rows stages the whole row in LDS; wider rows go to renet_topk_rows_wide
TOPK_ROWS_WIDE_MAX_C = 1 << 20          # RENET_TOPK_ROWS_WIDE_MAX_C of include/renet_hip.h
_topk_wide_ws = {}                      # device -> the workspace of renet_topk_rows_wide (the largest asked for so far)


def _topk_rows_front(what, scores, k, cols, start, count, keep, want_logp):
    """The checks and the outputs the two top-k entries share -> (n, C, k, ld, list arguments, idx, val, logp, n_valid)."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1):
        raise RenetHipError(what + ' needs a 2-D float32 device tensor with unit inner stride')
    n, c = scores.shape
    if cols is None and start is None and count is None:
        lists = [None, None, None, 0]
    elif cols is None or start is None or count is None or start.numel() != n or count.numel() != n:
        raise RenetHipError(what + ': a filter list is (cols, start [n], count [n])')
    else:                               # (an empty table has no storage to point at: no list)
        lists = [_i32(cols), _i32(start), _i32(count), cols.numel()] if cols.numel() else [None, None, None, 0]
    if keep is not None and keep.numel() != n:
        raise RenetHipError(what + ': shape mismatch')
    k = int(k)
    idx = torch.empty(n, k, device=scores.device, dtype=torch.int32)
    val = torch.empty(n, k, device=scores.device, dtype=torch.float32)
    logp = torch.empty(n, k, device=scores.device, dtype=torch.float32) if want_logp else None
    n_valid = torch.empty(n, device=scores.device, dtype=torch.int32)
    return n, c, k, max(_ld(scores), c) if n == 1 else _ld(scores), lists, idx, val, logp, n_valid


def topk_rows(scores, k, cols=None, start=None, count=None, keep=None, want_logp=True):
    """The k best candidates of every row of scores [n, C] (fp32, unit inner stride; not written) from ONE read of the scores
    -> (idx int32 [n, k], val [n, k], logp [n, k] or None, n_valid int32 [n]), by score descending, then column ascending
    (deterministic).  The candidates of row i are all columns minus cols[start[i] : start[i] + count[i]] (a range of a
    resident column table, filter_index.FilterIndex.ranges; int32), a listed column equal to keep[i] (int32 [n]) staying in;
    three Nones (or an empty table): no list.  logp = val - logsumexp(whole row), listed columns included.
    n_valid = min(k, candidates); the slots behind it hold idx -1, val -inf, logp -inf.  1 <= k <= 1024.
    C <= 32768: renet_topk_rows (the row staged in one CU's LDS); wider, up to 2^20 columns: renet_topk_rows_wide (the row in
    pieces, merged per row: topk_rows_wide below), with the same results."""
    if scores.dim() == 2 and scores.shape[1] > TOPK_ROWS_MAX_C:
        return topk_rows_wide(scores, k, cols, start, count, keep, want_logp)
    n, c, k, ld, lists, idx, val, logp, n_valid = _topk_rows_front('topk_rows', scores, k, cols, start, count, keep,
                                                                   want_logp)
    t0 = _timed()
    _check(lib().renet_topk_rows(scores.data_ptr(), ld, n, c, k, *lists, _i32(keep), idx.data_ptr(), val.data_ptr(),
                                 _f32(logp), n_valid.data_ptr(), _stream()), 'topk_rows')
    _timed_end(t0, 'topk_rows', nbytes=float(n * c * 4))
    return idx, val, logp, n_valid


def topk_rows_wide(scores, k, cols=None, start=None, count=None, keep=None, want_logp=True, stage_cols=0):
    """renet_topk_rows_wide: topk_rows' arguments and results for any C <= 2^20, the row taken in pieces of stage_cols columns
    (0: the library's choice; else 64 .. 32768 -- tests make the pieces small).  The workspace (the pieces' entries: n *
    pieces * (min(k, stage_cols) * 8 + 24) bytes) is kept per device, grown to the largest size asked for, and reused by every
    later call: calls on one device must be ordered on one stream."""
    n, c, k, ld, lists, idx, val, logp, n_valid = _topk_rows_front('topk_rows_wide', scores, k, cols, start, count, keep,
                                                                   want_logp)
    stage_cols = int(stage_cols)
    nbytes = lib().renet_topk_rows_wide_workspace(n, c, k, stage_cols)
    ws = _topk_wide_ws.get(scores.device)
    if nbytes and (ws is None or ws.numel() * 8 < nbytes):
        ws = _topk_wide_ws[scores.device] = torch.empty(nbytes // 8, device=scores.device, dtype=torch.int64)
    t0 = _timed()
    _check(lib().renet_topk_rows_wide(scores.data_ptr(), ld, n, c, k, *lists, _i32(keep), idx.data_ptr(), val.data_ptr(),
                                      _f32(logp), n_valid.data_ptr(), stage_cols, None if ws is None else ws.data_ptr(),
                                      nbytes, _stream()), 'topk_rows_wide')
    _timed_end(t0, 'topk_rows_wide', nbytes=float(n * c * 4))
    return idx, val, logp, n_valid


def _block_ld(scores):
    """Row stride of a [rows, C] block (a one-row block may carry any stride)."""
    return max(_ld(scores), scores.shape[1]) if scores.shape[0] == 1 else _ld(scores)


def query_histories(ent_ptr, snap_t, num_ent, history_len, ent, as_of):
    """renet_query_histories: the history windows of n arbitrary queries against a resident history index.  ent_ptr /
    snap_t: per role (0 subject, 1 object histories) the int32 device arrays ent_ptr [num_ent + 1] and snap_t; ent int32
    [2, n] (subjects, objects), as_of int32 [n] -> win int32 [2, 2, n]: win[0] = h_first[2][n], win[1] = h_count[2][n], equal
    to preprocess.HistoryIndex.lookup element for element; an entity outside [0, num_ent) gets (0, 0).  ONE launch."""
    if not (ent.dim() == 2 and ent.shape[0] == 2 and as_of.dim() == 1 and as_of.shape[0] == ent.shape[1]):
        raise RenetHipError('query_histories: ent must be [2, n] and as_of [n]')
    for r in (0, 1):
        if ent_ptr[r].numel() != int(num_ent) + 1:
            raise RenetHipError('query_histories: ent_ptr must hold num_ent + 1 entries')
    n = int(as_of.shape[0])
    win = torch.empty(2, 2, n, device=ent.device, dtype=torch.int32)
    t0 = _timed()
    _check(lib().renet_query_histories(_i32(ent_ptr[0], 'ent_ptr'), _i32(ent_ptr[1], 'ent_ptr'), _i32(snap_t[0], 'snap_t'),
                                       _i32(snap_t[1], 'snap_t'), int(num_ent), int(history_len), _i32(ent, 'ent'),
                                       _i32(as_of, 'as_of'), n, win[0].data_ptr(), win[1].data_ptr(), _stream()),
           'query_histories')
    _timed_end(t0, 'query_histories', nbytes=float(n * 28))
    return win


def store_append(old, q_ent, num_ent, history_len, new, cap_snaps):
    """renet_store_append: the history index of ONE role after the facts `new` were observed.  old = (ent_ptr [num_ent + 1],
    snap_t, snap_ptr, nbr_o, h_first, h_count) and q_ent [n_quads] (the role's entity of every old quadruple), int32 device
    tensors that are only read; new = int32 [4, m]: the new facts' entity, time, neighbour and input position, sorted stably
    by (entity, time, input order); cap_snaps = the snapshots of the longer index (any value in [n_snaps, n_snaps + m]: no
    store goes past it) -> ((ent_ptr, snap_t, snap_ptr, nbr_o, h_first, h_count) freshly allocated, totals int32 [2] on the
    device = (snapshots of the longer index, of which opened): the tables are complete when totals[0] == cap_snaps).  Equal
    to preprocess.HistoryIndex.appended array for array.  On the current stream; nothing is read back."""
    ent_ptr, snap_t, snap_ptr, nbr_o, h_first, h_count = old
    num_ent, cap = int(num_ent), int(cap_snaps)
    n_snaps, nq = int(snap_t.numel()), int(q_ent.numel())
    if not (new.dim() == 2 and new.shape[0] == 4):
        raise RenetHipError('store_append: new must be [4, m]')
    m = int(new.shape[1])
    if ent_ptr.numel() != num_ent + 1 or snap_ptr.numel() != n_snaps + 1 or \
            any(int(a.numel()) != nq for a in (nbr_o, h_first, h_count)):
        raise RenetHipError('store_append: the old index does not fit num_ent / its own lengths')
    dev = ent_ptr.device
    mk = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
    out = (mk(num_ent + 1), mk(cap), mk(cap + 1), mk(nq + m), mk(nq + m), mk(nq + m))
    totals = mk(2)
    nbytes = lib().renet_store_append_workspace(num_ent, m)
    ws = mk(nbytes // 4 + 64)
    t0 = _timed()
    _check(lib().renet_store_append(*[_i32(a, 'old index') for a in old], _i32(q_ent, 'q_ent'), num_ent, n_snaps, nq,
                                    int(history_len), *[_i32(new[k], 'new') if m else None for k in range(4)], m, cap,
                                    *[_i32(a) for a in out], totals.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           'store_append')
    _timed_end(t0, 'store_append', nbytes=float((num_ent + 2 * n_snaps + 4 * nq) * 8))
    return out, totals


def append_i32(old, add, n_old=None):
    """renet_append_i32: a fresh int32 tensor old[:n_old] ++ add (n_old: None = all of old); both int32 device tensors."""
    n_old = int(old.numel()) if n_old is None else int(n_old)
    if not 0 <= n_old <= old.numel():
        raise RenetHipError('append_i32: n_old outside the old array')
    n_add = int(add.numel())
    out = torch.empty(n_old + n_add, device=old.device, dtype=torch.int32)
    _check(lib().renet_append_i32(_i32(old) if n_old else None, n_old, _i32(add) if n_add else None, n_add,
                                  out.data_ptr(), _stream()), 'append_i32')
    return out


def pair_append(old, ent_ptr, snap_ptr, ent_ptr_new, snap_ptr_new, num_ent, new):
    """renet_pair_append: the pair tables of ONE role after the facts `new` were appended.  old = (p_rel, p_other, p_t) [n];
    ent_ptr / snap_ptr of the old history index and ent_ptr_new / snap_ptr_new of the longer one (store_append's outputs);
    new = int32 [4, m]: the new facts' entity, relation, partner and time, sorted by that key -> (p_rel, p_other, p_t)
    [n + m], freshly allocated.  Equal to preprocess.PairIndex.appended array for array.  On the current stream; nothing is
    read back; the old tables stay valid."""
    p_rel, p_other, p_t = old
    num_ent, n = int(num_ent), int(p_rel.numel())
    if not (new.dim() == 2 and new.shape[0] == 4):
        raise RenetHipError('pair_append: new must be [4, m]')
    m = int(new.shape[1])
    if p_other.numel() != n or p_t.numel() != n or ent_ptr.numel() != num_ent + 1 or ent_ptr_new.numel() != num_ent + 1:
        raise RenetHipError('pair_append: the old tables do not fit num_ent / their own lengths')
    out = tuple(torch.empty(n + m, device=ent_ptr.device, dtype=torch.int32) for _ in range(3))
    t0 = _timed()
    _check(lib().renet_pair_append(*[_i32(a, 'pair table') if n else None for a in old], n, _i32(ent_ptr, 'ent_ptr'),
                                   _i32(snap_ptr, 'snap_ptr'), int(snap_ptr.numel()) - 1, _i32(ent_ptr_new, 'ent_ptr'),
                                   _i32(snap_ptr_new, 'snap_ptr'), int(snap_ptr_new.numel()) - 1, num_ent,
                                   *[_i32(new[k], 'new') if m else None for k in range(4)], m,
                                   *[a.data_ptr() for a in out], _stream()), 'pair_append')
    _timed_end(t0, 'pair_append', nbytes=float((2 * n + m) * 12))
    return out


RECURRENCE_MAX_C = 1 << 20              # RENET_RECURRENCE_MAX_C of include/renet_hip.h


def recurrence_mix_rows(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, alpha, inv_half_life=0.0,
                        num_cols=None, want_stats=False):
    """renet_recurrence_mix_rows, one direction: out [n, C] (fp32, fresh) with
        out[i, o] = log((1 - a_i) softmax(logits[i])[o] + a_i w_i[o] / W_i)
    for the queries (ent, rel, t, as_of) (int32 device [n], as_of <= t), w_i[o] the 2^(-(t - t') inv_half_life)-weighted
    count of the facts (ent_i, rel_i, o, t' < as_of_i) of the role's pair tables `tables` = (p_rel, p_other, p_t), W_i their
    sum and a_i = alpha where W_i > 0, else 0.  logits [n, C] (fp32, unit inner stride; not written) or None: uniform rows of
    num_cols columns.  ent_ptr / snap_ptr: the role's resident history index.  0 <= alpha < 1.  A row of out is a normalised
    log-probability row: rank_rows3 and topk_rows read it as they read logits.  want_stats: -> (out, stats int32 [n, 2] =
    (distinct partners, facts counted), W fp32 [n])."""
    return _recurrence_mix(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, alpha, None, inv_half_life,
                           num_cols, want_stats)


def recurrence_mix_rows_gated(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, alpha_row, inv_half_life=0.0,
                              num_cols=None, want_stats=False, check=True):
    """renet_recurrence_mix_rows_gated: recurrence_mix_rows with one gate per row, alpha_row (fp32 device [n], each in
    [0, 1)) -- a_i = alpha_row[i] where W_i > 0, else 0.  check: read alpha_row's range back (one synchronisation) and refuse
    a gate outside [0, 1) before the launch; a caller that built the gates from a checked table passes False."""
    if not (torch.is_tensor(alpha_row) and alpha_row.is_cuda and alpha_row.dtype == torch.float32 and
            alpha_row.is_contiguous() and alpha_row.numel() == ent.numel()):
        raise RenetHipError('recurrence_mix_rows_gated: alpha_row must be a contiguous float32 device tensor, one per row')
    if check and alpha_row.numel():
        lo, hi = (float(v) for v in torch.aminmax(alpha_row.detach()))
        if not (lo >= 0.0 and hi < 1.0):
            raise RenetHipError('recurrence_mix_rows_gated: every gate must lie in [0, 1)')
    return _recurrence_mix(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, None, alpha_row.detach(),
                           inv_half_life, num_cols, want_stats)


def _row_floats(x, n, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n):
        raise RenetHipError('%s must be a contiguous float32 device tensor, one per row' % what)
    return x.detach()


def recurrence_mix_rows_decay(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, alpha_row, ihl_row,
                              num_cols=None, want_stats=False, check=True):
    """renet_recurrence_mix_rows_decay: recurrence_mix_rows_gated with one DECAY per row as well, ihl_row (fp32 device [n],
    each finite and >= 0) in inv_half_life's place -- w_i[o] sums 2^(-(t - t') ihl_row[i]).  A constant ihl_row gives the gated
    entry's bits.  check: read both ranges back (one synchronisation each) and refuse a gate outside [0, 1) or a decay that
    is negative or not finite before the launch; a caller that built both from checked tables passes False."""
    n = int(ent.numel())
    alpha_row = _row_floats(alpha_row, n, 'recurrence_mix_rows_decay: alpha_row')
    ihl_row = _row_floats(ihl_row, n, 'recurrence_mix_rows_decay: ihl_row')
    if check and n:
        lo, hi = (float(v) for v in torch.aminmax(alpha_row))
        if not (lo >= 0.0 and hi < 1.0):
            raise RenetHipError('recurrence_mix_rows_decay: every gate must lie in [0, 1)')
        lo, hi = (float(v) for v in torch.aminmax(ihl_row))
        if not (lo >= 0.0 and hi < float('inf')):
            raise RenetHipError('recurrence_mix_rows_decay: every decay must be finite and >= 0')
    return _recurrence_mix(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, None, alpha_row, 0.0, num_cols,
                           want_stats, ihl_row=ihl_row)


def _recurrence_mix(ent, rel, t, as_of, tables, ent_ptr, snap_ptr, num_ent, logits, alpha, alpha_row, inv_half_life, num_cols,
                    want_stats, ihl_row=None):
    n = int(ent.numel())
    if any(int(a.numel()) != n for a in (rel, t, as_of)):
        raise RenetHipError('recurrence_mix_rows: ent, rel, t and as_of must have one entry per row')
    if logits is not None:
        if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1):
            raise RenetHipError('recurrence_mix_rows needs a 2-D float32 device tensor with unit inner stride')
        if logits.shape[0] != n or (num_cols is not None and int(num_cols) != logits.shape[1]):
            raise RenetHipError('recurrence_mix_rows: shape mismatch')
        c, ld = int(logits.shape[1]), (max(_ld(logits), logits.shape[1]) if n == 1 else _ld(logits))
    else:
        if num_cols is None:
            raise RenetHipError('recurrence_mix_rows: uniform rows need num_cols')
        c, ld = int(num_cols), int(num_cols)
    p_rel, p_other, p_t = tables
    nf = int(p_rel.numel())
    if p_other.numel() != nf or p_t.numel() != nf or ent_ptr.numel() != int(num_ent) + 1:
        raise RenetHipError('recurrence_mix_rows: the pair tables do not fit num_ent / their own lengths')
    dev = ent.device
    out = torch.empty(n, c, device=dev, dtype=torch.float32)
    stats = torch.empty(n, 2, device=dev, dtype=torch.int32) if want_stats else None
    wsum = torch.empty(n, device=dev, dtype=torch.float32) if want_stats else None
    t0 = _timed()
    front = (_i32(ent, 'ent'), _i32(rel, 'rel'), _i32(t, 't'), _i32(as_of, 'as_of'), n,
             *[_i32(a, 'pair table') if nf else None for a in tables], nf, _i32(ent_ptr, 'ent_ptr'),
             _i32(snap_ptr, 'snap_ptr'), int(snap_ptr.numel()) - 1, int(num_ent),
             None if logits is None else logits.data_ptr(), ld, c)
    back = (float(inv_half_life), out.data_ptr(), _i32(stats), _f32(wsum), _stream())
    if ihl_row is not None:
        _check(lib().renet_recurrence_mix_rows_decay(*front, _f32(alpha_row, 'alpha_row'), _f32(ihl_row, 'ihl_row'), *back[1:]),
               'recurrence_mix_rows_decay')
    elif alpha_row is None:
        _check(lib().renet_recurrence_mix_rows(*front, float(alpha), *back), 'recurrence_mix_rows')
    else:
        _check(lib().renet_recurrence_mix_rows_gated(*front, _f32(alpha_row, 'alpha_row'), *back), 'recurrence_mix_rows_gated')
    _timed_end(t0, 'recurrence_mix_rows', nbytes=float(n * c * (4 if logits is None else 12)))
    return (out, stats, wsum) if want_stats else out


def recurrence_gold_rows(ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_cols, inv_half_life=0.0):
    """renet_recurrence_gold_rows, one direction: -> (q, W), fp32 device [n]: W_i the W of recurrence_mix_rows (its stats_w
    bit for bit) and q_i = w_i[gold_i] / W_i, the prior's mass on the column gold_i (int32 device [n]); both 0 where the pair
    has no history before as_of_i or the entity lies outside [0, num_ent), q_i = 0 where gold_i lies outside [0, num_cols)."""
    n = int(ent.numel())
    if any(int(a.numel()) != n for a in (rel, t, as_of, gold)):
        raise RenetHipError('recurrence_gold_rows: ent, rel, t, as_of and gold must have one entry per row')
    p_rel, p_other, p_t = tables
    nf = int(p_rel.numel())
    if p_other.numel() != nf or p_t.numel() != nf or ent_ptr.numel() != int(num_ent) + 1:
        raise RenetHipError('recurrence_gold_rows: the pair tables do not fit num_ent / their own lengths')
    q = torch.empty(n, device=ent.device, dtype=torch.float32)
    w = torch.empty(n, device=ent.device, dtype=torch.float32)
    t0 = _timed()
    _check(lib().renet_recurrence_gold_rows(_i32(ent, 'ent'), _i32(rel, 'rel'), _i32(t, 't'), _i32(as_of, 'as_of'),
                                            _i32(gold, 'gold'), n, *[_i32(a, 'pair table') if nf else None for a in tables],
                                            nf, _i32(ent_ptr, 'ent_ptr'), _i32(snap_ptr, 'snap_ptr'),
                                            int(snap_ptr.numel()) - 1, int(num_ent), int(num_cols), float(inv_half_life),
                                            q.data_ptr(), w.data_ptr(), _stream()), 'recurrence_gold_rows')
    _timed_end(t0, 'recurrence_gold_rows', nbytes=float(n * 28))
    return q, w


def recurrence_gold_rows_decay(ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_cols, ihl_row):
    """renet_recurrence_gold_rows_decay, one direction: -> (q, W, dq), fp32 device [n]: recurrence_gold_rows with the decay of
    row i taken from ihl_row (fp32 device [n], each finite and >= 0: the caller's to keep) and dq_i = d q_i / d ihl_row[i] =
    -ln2 (GD W - G WD) / W^2, exactly 0 where W_i = 0 or the gold column has no counted fact.  A constant ihl_row gives the
    (q, W) of recurrence_gold_rows bit for bit."""
    n = int(ent.numel())
    if any(int(a.numel()) != n for a in (rel, t, as_of, gold)):
        raise RenetHipError('recurrence_gold_rows_decay: ent, rel, t, as_of and gold must have one entry per row')
    ihl_row = _row_floats(ihl_row, n, 'recurrence_gold_rows_decay: ihl_row')
    p_rel, p_other, p_t = tables
    nf = int(p_rel.numel())
    if p_other.numel() != nf or p_t.numel() != nf or ent_ptr.numel() != int(num_ent) + 1:
        raise RenetHipError('recurrence_gold_rows_decay: the pair tables do not fit num_ent / their own lengths')
    q, w, dq = (torch.empty(n, device=ent.device, dtype=torch.float32) for _ in range(3))
    t0 = _timed()
    _check(lib().renet_recurrence_gold_rows_decay(_i32(ent, 'ent'), _i32(rel, 'rel'), _i32(t, 't'), _i32(as_of, 'as_of'),
                                                  _i32(gold, 'gold'), n, *[_i32(a, 'pair table') if nf else None for a in tables],
                                                  nf, _i32(ent_ptr, 'ent_ptr'), _i32(snap_ptr, 'snap_ptr'),
                                                  int(snap_ptr.numel()) - 1, int(num_ent), int(num_cols),
                                                  _f32(ihl_row, 'ihl_row'), q.data_ptr(), w.data_ptr(), dq.data_ptr(),
                                                  _stream()), 'recurrence_gold_rows_decay')
    _timed_end(t0, 'recurrence_gold_rows', nbytes=float(n * 36))
    return q, w, dq


JOINT_MAX_RELS = 1024                  # renet_joint_mix_rows, renet_joint_gold_rows: R at most this


def _joint_gold_front(what, ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_rels, num_cols):
    n = int(ent.numel())
    if any(int(a.numel()) != n for a in (rel, t, as_of, gold)):
        raise RenetHipError('%s: ent, rel, t, as_of and gold must have one entry per row' % what)
    if not 1 <= int(num_rels) <= JOINT_MAX_RELS:
        raise RenetHipError('%s: num_rels must lie in [1, %d]' % (what, JOINT_MAX_RELS))
    p_rel, p_other, p_t = tables
    nf = int(p_rel.numel())
    if p_other.numel() != nf or p_t.numel() != nf or ent_ptr.numel() != int(num_ent) + 1:
        raise RenetHipError('%s: the pair tables do not fit num_ent / their own lengths' % what)
    return n, (_i32(ent, 'ent'), _i32(rel, 'rel'), _i32(t, 't'), _i32(as_of, 'as_of'), _i32(gold, 'gold'), n,
               *[_i32(a, 'pair table') if nf else None for a in tables], nf, _i32(ent_ptr, 'ent_ptr'),
               _i32(snap_ptr, 'snap_ptr'), int(snap_ptr.numel()) - 1, int(num_ent), int(num_rels), int(num_cols))


def joint_gold_rows(ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_rels, num_cols, inv_half_life=0.0):
    """renet_joint_gold_rows, one direction: -> (q, W), fp32 device [n].  Row i is the given entity ent_i with the GOLD relation
    rel_i and the gold partner gold_i (int32 device [n]); W_i is the entity-wide W of joint_mix_rows (fp32 of its mass, bit for
    bit) and q_i = w_i[rel_i, gold_i] / W_i the prior's mass on the gold PAIR.  Both 0 where the entity has no history before
    as_of_i or lies outside [0, num_ent); q_i = 0 where gold_i lies outside [0, num_cols) or rel_i outside [0, num_rels).
    num_rels in [1, 1024]."""
    n, front = _joint_gold_front('joint_gold_rows', ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_rels,
                                 num_cols)
    q = torch.empty(n, device=ent.device, dtype=torch.float32)
    w = torch.empty(n, device=ent.device, dtype=torch.float32)
    t0 = _timed()
    _check(lib().renet_joint_gold_rows(*front, float(inv_half_life), q.data_ptr(), w.data_ptr(), _stream()), 'joint_gold_rows')
    _timed_end(t0, 'joint_gold_rows', nbytes=float(n * 28))
    return q, w


def joint_gold_rows_decay(ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent, num_rels, num_cols, ihl_row):
    """renet_joint_gold_rows_decay, one direction: -> (q, W, dq), fp32 device [n]: joint_gold_rows with the decay of row i taken
    from ihl_row (fp32 device [n], each finite and >= 0: the caller's to keep) and dq_i = d q_i / d ihl_row[i], exactly 0 where
    W_i = 0 or the gold pair has no counted fact.  A constant ihl_row gives the (q, W) of joint_gold_rows bit for bit."""
    n, front = _joint_gold_front('joint_gold_rows_decay', ent, rel, t, as_of, gold, tables, ent_ptr, snap_ptr, num_ent,
                                 num_rels, num_cols)
    ihl_row = _row_floats(ihl_row, n, 'joint_gold_rows_decay: ihl_row')
    q, w, dq = (torch.empty(n, device=ent.device, dtype=torch.float32) for _ in range(3))
    t0 = _timed()
    _check(lib().renet_joint_gold_rows_decay(*front, _f32(ihl_row, 'ihl_row'), q.data_ptr(), w.data_ptr(), dq.data_ptr(),
                                             _stream()), 'joint_gold_rows_decay')
    _timed_end(t0, 'joint_gold_rows', nbytes=float(n * 36))
    return q, w, dq


def joint_row_offsets(scores, num_rels, logits_r):
    """renet_joint_row_offsets on the block scores [G * R, C] (fp32, unit inner stride; not written) and the relation head's
    logits_r [G, R]: -> off [G * R] (fp32) with off[g * R + r] = logsoftmax(logits_r[g])[r] - logsumexp(scores[g * R + r]),
    both in fp64, rounded once.  The joint log-probability of the pair (r, c) of group g is scores[g * R + r, c] +
    off[g * R + r] as one fp32 addition; it is never stored.  R <= 1024."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1):
        raise RenetHipError('joint_row_offsets needs a 2-D float32 device tensor with unit inner stride')
    rows, c = scores.shape
    r = int(num_rels)
    g = rows // max(r, 1)
    if r < 1 or rows != g * r or tuple(logits_r.shape) != (g, r) or logits_r.dtype != torch.float32 or \
            not logits_r.is_cuda or logits_r.stride(1) != 1:
        raise RenetHipError('joint_row_offsets: shape mismatch')
    off = torch.empty(rows, device=scores.device, dtype=torch.float32)
    t0 = _timed()
    _check(lib().renet_joint_row_offsets(scores.data_ptr(), _block_ld(scores), g, r, c, logits_r.data_ptr(),
                                         _block_ld(logits_r), off.data_ptr(), _stream()), 'joint_row_offsets')
    _timed_end(t0, 'joint_row_offsets', nbytes=float(rows * c * 4))
    return off


def joint_mix_rows(scores, num_rels, off, ent, t, as_of, tables, ent_ptr, snap_ptr, num_ent, alpha, inv_half_life=0.0,
                   mass=None):
    """renet_joint_mix_rows: the recurrence prior mixed into the joint block scores [G * R, C] (fp32, unit inner stride) and its
    offsets off [G * R] (joint_row_offsets) IN PLACE -> mass (fp64 device [G]; the tensor given, or a fresh one).  Group g is the
    history of the entity ent[g] at t[g] as of as_of[g] (int32 device [G]); tables = (p_rel, p_other, p_t), ent_ptr and snap_ptr
    those of the GIVEN entity's role.  With w[r, c] the 2^(-(t - t') inv_half_life)-weighted count of the facts (ent, r, c, t' <
    as_of), W (= mass[g]) their sum over every relation and a = alpha where W > 0, else 0, and J = scores + off[row] in fp32:
        M = J + log1p(-a) for a pair without a counted fact,  M = log((1 - a) exp(J) + a w[r, c] / W) for one with,
    in fp64, rounded once.  Where a > 0 (and for alpha = 0 where W > 0) scores holds M and off is 0 afterwards, so that
    joint_rank_rows / topk_rows + off read the mixed joint unchanged; a group without history keeps rows and off bit for bit.
    0 <= alpha < 1; R <= 1024."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1):
        raise RenetHipError('joint_mix_rows needs a 2-D float32 device tensor with unit inner stride')
    rows, c = scores.shape
    r = int(num_rels)
    g = int(ent.numel())
    if r < 1 or rows != g * r or off.numel() != rows or t.numel() != g or as_of.numel() != g:
        raise RenetHipError('joint_mix_rows: shape mismatch')
    p_rel, p_other, p_t = tables
    nf = int(p_rel.numel())
    if p_other.numel() != nf or p_t.numel() != nf or ent_ptr.numel() != int(num_ent) + 1:
        raise RenetHipError('joint_mix_rows: the pair tables do not fit num_ent / their own lengths')
    if mass is None:
        mass = torch.empty(g, device=scores.device, dtype=torch.float64)
    elif not (mass.is_cuda and mass.dtype == torch.float64 and mass.is_contiguous() and mass.numel() == g):
        raise RenetHipError('joint_mix_rows: mass must be a contiguous float64 device tensor, one per group')
    t0 = _timed()
    _check(lib().renet_joint_mix_rows(_i32(ent, 'ent'), _i32(t, 't'), _i32(as_of, 'as_of'), g,
                                      *[_i32(a, 'pair table') if nf else None for a in tables], nf, _i32(ent_ptr, 'ent_ptr'),
                                      _i32(snap_ptr, 'snap_ptr'), int(snap_ptr.numel()) - 1, int(num_ent), scores.data_ptr(),
                                      _block_ld(scores), r, int(c), _f32(off, 'off'), float(alpha), float(inv_half_life),
                                      mass.data_ptr(), _stream()), 'joint_mix_rows')
    _timed_end(t0, 'joint_mix_rows', nbytes=float(rows * c * 8))
    return mass


SELECT_EVENTS_MAX = 1024               # renet_select_events: R, k and num_k at most this


def select_events(ent, val, off, g_ent, g_lprior, g_mult, num_k, carry=None, workspace=None):
    """renet_select_events: the global choice of the generated events over one block and the winners carried so far.
    ent int32 / val fp32 [G * R, k] (topk_rows' idx / val), off fp32 [G * R] (joint_row_offsets), g_ent int32 / g_lprior fp32 /
    g_mult int32 [G] (G = 0: the six may be None); carry: None or an earlier result -> (given, rel, other int32 [num_k], val
    fp32 [num_k], mult int32 [num_k], n int32 [1]), fresh device tensors: the shortest prefix, by (V descending, carry first,
    flat position), whose summed multiplicity reaches num_k, V = (val + off[row]) + g_lprior[g] in fp32; the slots behind n
    hold -1, -1, -1, -inf, 0.  workspace: an int64 device tensor to use (None: allocated here).  Nothing is read back."""
    num_k = int(num_k)
    if g_ent is None:
        g, r, k = 0, 1, 1
        if carry is None:
            raise RenetHipError('select_events: no block and no carry')
        dev = carry[0].device
    else:
        g = int(g_ent.numel())
        rows, k = (int(x) for x in ent.shape)
        r = rows // max(g, 1)
        dev = g_ent.device
        if ent.dim() != 2 or g < 1 or rows != g * r or tuple(val.shape) != (rows, k) or off.numel() != rows or \
                g_lprior.numel() != g or g_mult.numel() != g:
            raise RenetHipError('select_events: shape mismatch')
    if carry is not None and (len(carry) != 6 or any(int(c.numel()) != num_k for c in carry[:5]) or carry[5].numel() != 1):
        raise RenetHipError('select_events: a carry is an earlier result for the same num_k')
    nbytes = lib().renet_select_events_workspace(g, r, k, num_k)
    if workspace is None or workspace.numel() * 8 < nbytes:
        workspace = torch.empty(max(nbytes // 8, 1), device=dev, dtype=torch.int64)
    n_out = max(num_k, 0)
    out = tuple(torch.empty(n_out, device=dev, dtype=torch.int32) for _ in range(3)) + \
        (torch.empty(n_out, device=dev, dtype=torch.float32), torch.empty(n_out, device=dev, dtype=torch.int32),
         torch.empty(1, device=dev, dtype=torch.int32))
    ptr = lambda c, j: None if c is None else (_f32(c[j], 'carry') if j == 3 else _i32(c[j], 'carry'))
    blk = [None] * 6 if g == 0 else [_i32(ent, 'ent'), _f32(val, 'val'), _f32(off, 'off'), _i32(g_ent, 'g_ent'),
                                     _f32(g_lprior, 'g_lprior'), _i32(g_mult, 'g_mult')]
    t0 = _timed()
    _check(lib().renet_select_events(*blk, g, r, k, num_k, *[ptr(carry, j) for j in range(6)],
                                     *[ptr(out, j) for j in range(6)], workspace.data_ptr(), workspace.numel() * 8,
                                     _stream()), 'select_events')
    _timed_end(t0, 'select_events', nbytes=float(g * r * min(k, max(num_k, 1)) * 8 * 7))
    return out


def joint_rank_rows(scores, num_rels, off, group, gold_r, gold_c, cols_a=None, start_a=None, count_a=None, cols_t=None,
                    start_t=None, count_t=None):
    """renet_joint_rank_rows: Q queries rank their gold pair (gold_r[q], gold_c[q]) among the R * C pairs of group[q] of the
    block scores [G * R, C] (not written) on the fp32 values J = scores + off[row] (off [G * R]: joint_row_offsets, or any
    fp32 array) -> (counts int64 [6, Q], at_gold fp32 [Q, R], listed int32 [2, Q, R], rows int32 [6, Q, R]).
    counts = raw (greater, equal), filtered (greater, equal), time_filtered (greater, equal) over all pairs -- the kernel's
    per-row counts `rows` summed over the R rows of a query; rank = greater + (equal - 1) / 2 + 1.  A setting's list is
    (cols, start [Q * R], count [Q * R]), row q * R + r the columns that are no candidates in relation row r of query q (a
    range of a resident column table, filter_index.FilterIndex.ranges; int32), the gold pair always staying; three Nones (or
    an empty table): no list.  A column may appear AT MOST ONCE in a row's list (FilterIndex deduplicates): a listed column's
    contribution is subtracted once per occurrence, so a repeated column would be undercounted.  at_gold[q, r] = J[group[q], r, gold_c[q]]; listed[0 / 1, q, r] = 1 where gold_c[q] is on list
    a / t of row (q, r).  group, gold_r, gold_c: int32 [Q], clamped into range by the kernel."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1):
        raise RenetHipError('joint_rank_rows needs a 2-D float32 device tensor with unit inner stride')
    rows, c = scores.shape
    r = int(num_rels)
    g = rows // max(r, 1)
    q = group.numel()
    if r < 1 or rows != g * r or off.numel() != rows or gold_r.numel() != q or gold_c.numel() != q:
        raise RenetHipError('joint_rank_rows: shape mismatch')
    lists = []
    for cols, start, count in ((cols_a, start_a, count_a), (cols_t, start_t, count_t)):
        if cols is None and start is None and count is None:
            lists += [None, None, None, 0]
            continue
        if cols is None or start is None or count is None or start.numel() != q * r or count.numel() != q * r:
            raise RenetHipError('joint_rank_rows: a filter list is (cols, start [Q * R], count [Q * R])')
        # (an empty table has no storage to point at: no list)
        lists += [_i32(cols), _i32(start), _i32(count), cols.numel()] if cols.numel() else [None, None, None, 0]
    per_row = torch.empty(6, q, r, device=scores.device, dtype=torch.int32)
    at_gold = torch.empty(q, r, device=scores.device, dtype=torch.float32)
    listed = torch.empty(2, q, r, device=scores.device, dtype=torch.int32)
    t0 = _timed()
    _check(lib().renet_joint_rank_rows(scores.data_ptr(), _block_ld(scores), g, c, r, _f32(off), q, _i32(group), _i32(gold_r),
                                       _i32(gold_c), *lists, per_row.data_ptr(), at_gold.data_ptr(), listed.data_ptr(),
                                       _stream()), 'joint_rank_rows')
    _timed_end(t0, 'joint_rank_rows', nbytes=float(q * r * c * 4))
    return per_row.sum(dim=-1), at_gold, listed, per_row


def joint_softmax(logits, num_rels, logits_r, prob_e):
    """logits [n * R, N] -> IN PLACE softmax(row) * softmax(logits_r[e])[r] * prob_e[e]  (model.py:205-209).  Any N (rows up
    to 32768 columns are staged in LDS, wider ones streamed twice); R <= 1024."""
    nr, n_ent = logits.shape
    n = nr // num_rels
    if nr != n * num_rels or tuple(logits_r.shape) != (n, num_rels) or prob_e.numel() != n:
        raise RenetHipError('joint_softmax: shape mismatch')
    _check(lib().renet_joint_softmax(logits.data_ptr(), _ld(logits), n, num_rels, n_ent, logits_r.data_ptr(),
                                     _ld(logits_r), _f32(prob_e), _stream()), 'joint_softmax')
    return logits


def topk_positive(x, k):
    """Top-k of every row of an fp32 matrix [n, M] -> (values [n, k], int64 indices [n, k]).  Exact selection by an
    order-preserving key (any sign; -0.0 == +0.0; NaNs rank below every number).  The k results come back UNSORTED and
    their slot order -- and which of several elements EQUAL to the k-th value is taken -- depends on the arrival order of
    atomics: sort the result where a deterministic order matters (model.py does not depend on it)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise RenetHipError('topk_positive needs a 2-D float32 device tensor with unit inner stride')
    n, m = x.shape
    vals = torch.empty(n, k, device=x.device, dtype=torch.float32)
    idx = torch.empty(n, k, device=x.device, dtype=torch.int64)
    nbytes = lib().renet_topk_workspace(n)
    ws = torch.empty(nbytes // 4 + 1, device=x.device, dtype=torch.int32)
    _check(lib().renet_topk_positive(x.data_ptr(), x.stride(0) if n > 1 else m, n, m, int(k), vals.data_ptr(),
                                     idx.data_ptr(), ws.data_ptr(), nbytes, _stream()), 'topk_positive')
    return vals, idx


def segment_pool_fwd(h, seg_ptr, num_graphs, is_max):
    d = h.shape[1]
    out = torch.empty(num_graphs, d, device=h.device, dtype=torch.float32)
    arg = torch.empty(num_graphs, d, device=h.device, dtype=torch.int32)
    _check(lib().renet_segment_pool_fwd(_f32(h), _i32(seg_ptr), num_graphs, d, int(is_max), _f32(out),
                                        _i32(arg), _stream()), 'segment_pool_fwd')
    return out, arg


def segment_pool_bwd(dout, seg_ptr, arg, num_graphs, is_max, n):
    d = dout.shape[1]
    dh = torch.empty(n, d, device=dout.device, dtype=torch.float32)
    _check(lib().renet_segment_pool_bwd(_f32(dout), _i32(seg_ptr), _i32(arg), num_graphs, d, int(is_max), n,
                                        _f32(dh), _stream()), 'segment_pool_bwd')
    return dh


def _host_i32(a):
    """Host pointer of a contiguous int32 numpy array (the caller keeps the array alive across the call)."""
    if a.dtype.name != 'int32' or not a.flags['C_CONTIGUOUS']:
        raise RenetHipError('host index arrays must be contiguous int32')
    return a.ctypes.data_as(c_void_p)


def nbr_pool_fwd(e, r, p, q, v, nb):
    """Neighbour pooling of graph.NeighbourBatch `nb` (device arrays + the host copy of seg_ptr) -> (out, stats, w):
    mean mode (p is None) out [S, 2D] = [mean E[nbr] | E[s]], stats = w = None; attention mode out [S, 3D] =
    [softmax-weighted sum | E[s] | R[r]], stats [S, 2] = (max, log-sum) per segment, w [nnz] the softmax weights."""
    attn = p is not None
    d = e.shape[1]
    out = torch.empty(nb.S, (3 if attn else 2) * d, device=e.device, dtype=torch.float32)
    stats = torch.empty(nb.S, 2, device=e.device, dtype=torch.float32) if attn else None
    w = torch.empty(nb.nnz, device=e.device, dtype=torch.float32) if attn else None
    t0 = _timed()
    _check(lib().renet_nbr_pool_fwd(_f32(e), _f32(r) if attn else None, _f32(p), _f32(q) if attn else None,
                                    _f32(v) if attn else None, _i32(nb.nbr), _i32(nb.seg_ptr), _host_i32(nb.seg_ptr_host),
                                    _i32(nb.seg_s), _i32(nb.seg_r), _i32(nb.seg_q), _i32(nb.out_row), nb.S, d, int(attn),
                                    _f32(out), _f32(stats), _f32(w), _stream()), 'nbr_pool_fwd')
    _timed_end(t0, 'nbr_pool_fwd', nbytes=float(nb.nnz * d * 4 * (2 if attn else 1) + out.numel() * 4))
    return out, stats, w


def nbr_pool_bwd(dout, out, e, p, q, v, w, nb):
    """-> (cE [nnz, D], cP [nnz, D] | None, dq_rows [S, D] | None, dv_rows [S, D] | None, ds_rows [S, D],
    dr_rows [S, D] | None): the contribution rows and per-segment partial rows of renet_nbr_pool_bwd."""
    attn = p is not None
    d = e.shape[1]

    def rows(n, on=True):
        return torch.empty(n, d, device=e.device, dtype=torch.float32) if on else None
    ce, cp = rows(nb.nnz), rows(nb.nnz, attn)
    dq, dv, ds, dr = rows(nb.S, attn), rows(nb.S, attn), rows(nb.S), rows(nb.S, attn)
    t0 = _timed()
    _check(lib().renet_nbr_pool_bwd(_f32(dout), _f32(out) if attn else None, _f32(e), _f32(p), _f32(q) if attn else None,
                                    _f32(v) if attn else None, _f32(w), _i32(nb.nbr), _i32(nb.seg_ptr),
                                    _host_i32(nb.seg_ptr_host), _i32(nb.seg_q), _i32(nb.out_row), nb.S, d, int(attn),
                                    _f32(ce), _f32(cp), _f32(dq), _f32(dv), _f32(ds), _f32(dr), _stream()), 'nbr_pool_bwd')
    _timed_end(t0, 'nbr_pool_bwd', nbytes=float(nb.nnz * d * 4 * (4 if attn else 1) + dout.numel() * 4))
    return ce, cp, dq, dv, ds, dr


def sumsq_partials(g, partial, slot0, n_slots):
    """partial[slot0 : slot0 + n_slots) = per-workgroup sums of squares of the flat fp32 region g (current stream)."""
    _check(lib().renet_sumsq_partials(_f32(g), g.numel(), partial.data_ptr() + 4 * slot0, int(n_slots), _stream()),
           'sumsq_partials')


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, max_norm, step, zero_grad=True, norm_out=None,
              grad_scale=1.0, presummed=None):
    """Fused clip + Adam + zero_grad on flat fp32 buffers (in place); the gradient is g * grad_scale.
    presummed = (partial, n): ||g||^2 is the sum of partial[0..n) (sumsq_partials per all-reduce bucket), no norm pass."""
    n = p.numel()
    if presummed is not None:
        part, n_part = presummed
        _check(lib().renet_adam_step_presummed(_f32(p), _f32(g), _f32(m), _f32(v), n, float(lr), float(beta1), float(beta2),
                                               float(eps), float(weight_decay), float(max_norm), float(grad_scale),
                                               int(step), int(zero_grad), _f32(part), int(n_part), _f32(norm_out),
                                               _stream()), 'adam_step_presummed')
        return
    nbytes = lib().renet_adam_workspace(n)
    ws = torch.empty(nbytes // 4, device=p.device, dtype=torch.float32)
    _check(lib().renet_adam_step_scaled(_f32(p), _f32(g), _f32(m), _f32(v), n, float(lr), float(beta1), float(beta2),
                                        float(eps), float(weight_decay), float(max_norm), float(grad_scale), int(step),
                                        int(zero_grad), ws.data_ptr(), nbytes, _f32(norm_out), _stream()), 'adam_step')
