"""CPU tests of the host side of renet_topk_rows_wide (the kernels: tests/test_gpu_topk_rows_wide.py): the entry in the header
and the binding, the workspace sizes -- pure host arithmetic: pieces and entries per piece --, and the refusals that come
back before any launch."""
import os

from helpers import ROOT


def test_wide_entry_is_declared_and_bound():
    import renet_hip as K
    hdr = open(os.path.join(ROOT, 'include', 'renet_hip.h')).read()
    assert 'int renet_topk_rows_wide(const float* scores, int ld, int n, int C, int k,' in hdr
    assert 'size_t renet_topk_rows_wide_workspace(int n, int C, int k, int stage_cols);' in hdr
    assert '#define RENET_TOPK_ROWS_WIDE_MAX_C (1 << 20)' in hdr and K.TOPK_ROWS_WIDE_MAX_C == 1 << 20
    assert {'renet_topk_rows_wide', 'renet_topk_rows_wide_workspace'} <= set(K.EXPORTS)
    narrow, wide = K._SIGNATURES['renet_topk_rows'][1], K._SIGNATURES['renet_topk_rows_wide'][1]
    assert wide[:len(narrow) - 1] == narrow[:-1] and len(wide) == len(narrow) + 3        # + stage_cols, workspace, its bytes


def test_workspace_sizes():
    """n * pieces * (min(k, piece width) * 8 + 24) bytes; the default split is even, into pieces of at most 15360 columns
    that start on multiples of 4."""
    import renet_hip as K
    ws = K.lib().renet_topk_rows_wide_workspace
    assert ws(4, 8, 3, 0) == 4 * 1 * (3 * 8 + 24)
    assert ws(2, 65536, 10, 0) == 2 * 5 * (10 * 8 + 24)                  # 5 pieces of 13108
    assert ws(1, 15360, 1024, 0) == 1024 * 8 + 24 and ws(1, 15361, 1024, 0) == 2 * (1024 * 8 + 24)
    assert ws(3, 300, 1000, 64) == 3 * 5 * (64 * 8 + 24)                 # a piece supplies at most its width
    assert ws(3, 1 << 20, 1024, 32768) == 3 * 32 * (1024 * 8 + 24)
    for bad in ((0, 8, 3, 0), (4, 0, 3, 0), (4, (1 << 20) + 1, 3, 0), (4, 8, 0, 0), (4, 8, 1025, 0), (4, 8, 3, 63), (4, 8, 3, 32769)):
        assert ws(*bad) == 0, bad


def test_refusals_come_before_any_launch():
    """Nothing here reaches a launch, so no device is needed (the pointers are never followed)."""
    import renet_hip as K
    fn, ptr = K.lib().renet_topk_rows_wide, 4096

    def call(n=4, C=8, ld=8, k=3, stage=0, w=ptr, wbytes=1 << 20, out=ptr):
        return fn(ptr, ld, n, C, k, None, None, None, 0, None, out, ptr, ptr, ptr, stage, w, wbytes, None)
    assert call(k=0) == -1 and call(k=1025) == -1 and call(ld=7) == -1 and call(n=-1) == -1 and call(C=0) == -1
    assert call(stage=63) == -1 and call(stage=32769) == -1 and call(out=None) == -1
    assert call(n=0, C=(1 << 20) + 1, ld=(1 << 20) + 1) == -2 and call(C=(1 << 20) + 1, ld=(1 << 20) + 1) == -2
    assert call(n=0) == 0
    need = K.lib().renet_topk_rows_wide_workspace(4, 8, 3, 0)
    assert call(wbytes=need - 1) == -3 and call(w=None) == -3 and call(w=ptr + 4, wbytes=need) == -3
