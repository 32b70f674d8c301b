"""Host statement of the counter-based dropout mask (re-net_amd/csrc/common.h: renet_mix64, make_drop, renet_drop4), written
from the text of the header and nothing else: no kernel is asked what the mask is.

One splitmix64 draw per group of 4 consecutive elements, keyed by (seed, group index):

    r      = mix64(seed * 0xD1342543DE82EF95 + g)            (uint64, wrapping)
    keep j = ((r >> 16 j) & 0xFFFF) >= thresh,  j = 0..3
    thresh = uint32(float32(p) * 65536 + 0.5)                 (float32 arithmetic; p <= 0 or thresh == 0: keep everything)
    scale  = float32(1) / (float32(1) - float32(p))

The multipliers are returned as float64 (0 or the float32 value of `scale`), so that float32(float64(x) * mult) is exactly
the fp32 product a kernel forms.  The layout wrappers state which group index each kernel keys an element by."""
import numpy as np

_M64 = (1 << 64) - 1
_KEY = 0xD1342543DE82EF95


def mix64(x):
    """splitmix64's output function for the Python int x (taken mod 2^64)."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _mix64_array(x):
    """mix64 over a uint64 array (array arithmetic on uint64 wraps silently)."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def drop_config(p):
    """-> (thresh, scale) of make_drop: thresh a Python int, scale the float64 value of the float32 1 / (1 - p)."""
    p32 = np.float32(p)
    if p32 <= 0:
        return 0, 1.0
    thresh = int(np.uint32(p32 * np.float32(65536.0) + np.float32(0.5)))
    return thresh, float(np.float32(1.0) / (np.float32(1.0) - p32))


def multipliers_at(seed, groups, p):
    """The 4 multipliers of each group index in `groups` (any integer array) -> float64 [len(groups), 4]."""
    groups = np.atleast_1d(np.asarray(groups)).astype(np.uint64).ravel()
    thresh, scale = drop_config(p)
    if thresh == 0:
        return np.ones((groups.size, 4))
    key = np.full(groups.shape, (int(seed) * _KEY) & _M64, dtype=np.uint64)
    r = _mix64_array(key + groups)
    shifts = np.array([0, 16, 32, 48], dtype=np.uint64)
    draw = (r[:, None] >> shifts[None, :]) & np.uint64(0xFFFF)
    return np.where(draw >= np.uint64(thresh), scale, 0.0)


def drop_multipliers(seed, first_group, n_groups, p):
    """Multipliers of the groups first_group .. first_group + n_groups - 1 -> float64 [4 * n_groups]."""
    g = np.uint64(int(first_group) & _M64) + np.arange(int(n_groups), dtype=np.uint64)
    return multipliers_at(seed, g, p).reshape(-1)


def _rows_mask(rows, width, seed, p):
    assert width % 4 == 0
    row = np.arange(rows, dtype=np.int64)[:, None]
    col4 = np.arange(width // 4, dtype=np.int64)[None, :]
    groups = row * (width // 4) + col4                       # group = row * width/4 + col/4
    return multipliers_at(seed, groups, p).reshape(rows, width)


def flat_mask(rows, d, seed, p):
    """A flat [rows, D] tensor (renet_dropout, the self-loop mask of rgcn_bwd_prep): group = row * D/4 + col/4."""
    return _rows_mask(rows, d, seed, p)


def x_mask(s, d, seed, p):
    """The packed GRU input X = [h2 | ent | rel | glob], keyed by its UNPADDED [S, 4D] layout: group = row * D + col/4."""
    return _rows_mask(s, 4 * d, seed, p)


def xr_mask(s, d, seed, p):
    """Xr = [h2 | ent | glob], keyed by its unpadded [S, 3D] layout: group = row * 3D/4 + col/4 (col counted in Xr, so
    the glob part is columns [2D, 3D) here although it is part 3 of X)."""
    return _rows_mask(s, 3 * d, seed, p)


def concat_mask(b, parts, d, seed, p):
    """feat = [a[ia] | hmid (| c[ic])] of concat3, [B, parts * D]: group = row * parts * D/4 + col/4."""
    return _rows_mask(b, parts * d, seed, p)
