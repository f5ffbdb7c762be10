"""The vectorised oracles against the per-vertex ones they stand in for."""
import numpy as np
import pytest

from oracles import (cdlp_oracle, cdlp_oracle_fast, coreness_oracle,
                     coreness_oracle_fast)


def multigraph(num_v, num_e, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, num_v - 5, num_e).astype(np.int64)
    dst = rng.integers(0, num_v - 5, num_e).astype(np.int64)
    # parallel arcs, self-loops, a star whose labels oscillate
    hub = np.full(40, num_v - 6, dtype=np.int64)
    leaves = np.arange(40, dtype=np.int64)
    lv = rng.integers(0, num_v - 5, 6).astype(np.int64)
    return (np.concatenate([src, src[:30], hub, lv]),
            np.concatenate([dst, dst[:30], leaves, lv]))


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("num_v,num_e,seed", [(60, 90, 1), (300, 1500, 2),
                                               (400, 700, 3)])
def test_cdlp_fast_equals_cdlp(num_v, num_e, seed, directed):
    src, dst = multigraph(num_v, num_e, seed)
    for iters in (1, 2, 7):
        assert np.array_equal(
            cdlp_oracle_fast(num_v, src, dst, iters, directed=directed),
            cdlp_oracle(num_v, src, dst, iters, directed=directed))
    lab, changed = cdlp_oracle_fast(num_v, src, dst, 4, directed=directed,
                                    return_changed=True)
    assert len(changed) == 4 and changed[0] > 0


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("num_v,num_e,seed", [(60, 90, 4), (300, 1500, 5),
                                               (400, 700, 6)])
def test_coreness_fast_equals_coreness(num_v, num_e, seed, directed):
    src, dst = multigraph(num_v, num_e, seed)
    assert np.array_equal(
        coreness_oracle_fast(num_v, src, dst, directed=directed),
        coreness_oracle(num_v, src, dst, directed=directed))
