"""The host statement of the dropout mask (tests/dropout_masks.py) against published and hand-computed splitmix64 values
and against its own definition: no GPU, no kernel."""
import warnings

import numpy as np
import pytest

import dropout_masks as DM


def test_mix64_matches_published_and_pure_python_values():
    assert DM.mix64(0) == 0xE220A8397B1DCDAF                      # first output of splitmix64 seeded with 0
    assert DM.mix64((1234567 * 0xD1342543DE82EF95 + 5) % (1 << 64)) == 0xD8B5CAEECE4749DC
    # the array form is the same function
    xs = [0, 1, 5, (1 << 64) - 1, (1 << 63) + 12345, (1234567 * 0xD1342543DE82EF95 + 5) % (1 << 64)]
    got = DM._mix64_array(np.array(xs, dtype=np.uint64))
    assert [int(v) for v in got] == [DM.mix64(x) for x in xs]


def test_threshold_and_scale_are_the_float32_values_of_the_header():
    assert DM.drop_config(0.0) == (0, 1.0)
    assert DM.drop_config(0.5) == (32768, 2.0)
    assert DM.drop_config(0.25)[0] == 16384
    t, s = DM.drop_config(0.2)
    assert t == 13107 and s == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.2)))
    assert np.float32(s) == s                                     # a float32 value


def test_multipliers_of_one_group_written_out_by_hand():
    seed, g, p = 1234567, 5, 0.5
    r = DM.mix64((seed * 0xD1342543DE82EF95 + g) % (1 << 64))
    assert r == 0xD8B5CAEECE4749DC
    want = [2.0 if ((r >> (16 * j)) & 0xFFFF) >= 32768 else 0.0 for j in range(4)]
    assert want == [0.0, 2.0, 2.0, 2.0]                           # 0x49DC, 0xCE47, 0xCAEE, 0xD8B5 against 0x8000
    assert DM.drop_multipliers(seed, g, 1, p).tolist() == want
    assert DM.drop_multipliers(seed, 3, 4, p)[8:12].tolist() == want          # first_group offsets the counter


@pytest.mark.parametrize('p,frac', [(0.5, 0.5008), (0.25, 0.2503), (0.2, 0.2003)])
def test_values_and_zero_fraction(p, frac):
    m = DM.drop_multipliers(1234567, 0, 200000, p)
    assert m.dtype == np.float64 and m.shape == (800000,)
    scale = DM.drop_config(p)[1]
    assert set(np.unique(m).tolist()) == {0.0, scale}
    assert abs(float((m == 0).mean()) - frac) < 0.005
    assert np.array_equal(DM.drop_multipliers(7, 0, 1000, 0.0), np.ones(4000))


def test_extreme_seeds_wrap_without_warnings_and_differ():
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        masks = [DM.drop_multipliers(seed, 0, 4096, 0.5) for seed in (0, (1 << 40) + 3, (1 << 64) - 1)]
        far = DM.drop_multipliers((1 << 64) - 1, (1 << 64) - 2, 4, 0.5)        # the counter wraps too
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(masks[i], masks[j])
    want = [DM.mix64(((((1 << 64) - 1) * 0xD1342543DE82EF95) + (1 << 64) - 2 + k) % (1 << 64)) for k in range(4)]
    bits = [2.0 if ((r >> (16 * j)) & 0xFFFF) >= 32768 else 0.0 for r in want for j in range(4)]
    assert far.tolist() == bits


def test_layout_wrappers_key_by_the_unpadded_row_major_group():
    s, d, seed, p = 5, 8, 99, 0.5
    for mask, width in ((DM.flat_mask(s, d, seed, p), d), (DM.x_mask(s, d, seed, p), 4 * d),
                        (DM.xr_mask(s, d, seed, p), 3 * d), (DM.concat_mask(s, 2, d, seed, p), 2 * d),
                        (DM.concat_mask(s, 3, d, seed, p), 3 * d)):
        assert mask.shape == (s, width)
        assert np.array_equal(mask.reshape(-1), DM.drop_multipliers(seed, 0, s * width // 4, p))
    # element (row 3, col 13) of X is element 1 of group 3 * D + 3
    assert DM.x_mask(s, d, seed, p)[3, 13] == DM.drop_multipliers(seed, 3 * d + 3, 1, p)[1]
