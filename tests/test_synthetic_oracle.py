"""The contract of the NumPy model of load_synthetic's edge stream
(tests/synthetic_oracle.py) itself: no engine, no GPU.
tests/test_gpu_synthetic_oracle.py holds the device generator to the model."""
import numpy as np
import pytest

from synthetic_oracle import (edge_int, fold_ids, mix64, mix64_int,
                              raw_stream, scale_of, scramble_ids,
                              scramble_params, synthetic_edges, thresholds,
                              weight_of_bits)


def test_mix64_known_answers():
    # splitmix64 from state 0: the first outputs of the published generator
    want = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    g = 0x9E3779B97F4A7C15
    for k, w in enumerate(want):
        assert mix64_int((k * g) & ((1 << 64) - 1)) == w
    z = np.array([(k * g) & ((1 << 64) - 1) for k in range(3)],
                 dtype=np.uint64)
    assert [int(x) for x in mix64(z)] == list(want)
    rng = np.random.default_rng(1)
    z = rng.integers(0, 1 << 64, size=200, dtype=np.uint64)
    assert [int(x) for x in mix64(z)] == [mix64_int(int(x)) for x in z]


def test_scale_and_thresholds():
    assert [scale_of(n) for n in (1, 2, 3, 4, 5, 4096, 4097, 20000)] == \
        [0, 1, 2, 2, 3, 12, 13, 15]
    # truncated, not rounded: 0.57 * 65536 = 37355.52
    assert thresholds() == (37355, 49807, 62259)
    assert thresholds(0.45, 0.25, 0.15) == (29491, 45875, 55705)


# prime, power of two, 2^k + 1, and the shapes of the GPU test
BIJECTION_NV = (3, 4, 5, 7, 4096, 4097, 10007, 65536, 65537, 20000, 6000,
                5000)


@pytest.mark.parametrize("nv", BIJECTION_NV)
def test_scramble_is_a_bijection_that_keeps_zero(nv):
    from math import gcd
    for seed in (0, 1, 7, 42, (1 << 63) + 5):
        scr_a, scr_b = scramble_params(nv, seed)
        assert gcd(scr_a, nv) == 1 and 2 <= scr_a and 0 <= scr_b < nv
        y = scramble_ids(np.arange(nv), nv, seed)
        assert np.array_equal(np.sort(y), np.arange(nv)), (nv, seed)
        assert y[0] == 0, (nv, seed)  # raw vertex 0 keeps id 0
        if nv > 4:  # it does move things
            assert (y != np.arange(nv)).sum() > nv // 2


def test_no_scramble_for_tiny_graphs_or_on_request():
    assert scramble_params(1, 7) == (0, 0) == scramble_params(2, 7)
    assert scramble_params(20000, 7, scramble=False) == (0, 0)
    assert scramble_params(3, 1) == (2, 1)
    x = np.arange(2)
    assert np.array_equal(scramble_ids(x, 2, 7), x)
    x = np.arange(20000)
    assert np.array_equal(scramble_ids(x, 20000, 7, scramble=False), x)


@pytest.mark.parametrize("nv", (1, 2, 3))
def test_tiny_vertex_counts(nv):
    src, dst, w = synthetic_edges(nv, 50, 1, True)
    assert len(src) == len(dst) == len(w) == 50
    assert src.min() >= 0 and dst.min() >= 0
    assert src.max() < nv and dst.max() < nv
    if nv == 1:
        assert not src.any() and not dst.any()
    else:
        assert len(np.unique(src)) == nv and len(np.unique(dst)) == nv
    assert (w >= 1).all() and (w < 100).all()


SHAPES = ((20000, 160000, 7), (6000, 100000, 5), (4096, 40000, 3),
          (5000, 60000, 11), (4097, 30000, 2))


@pytest.mark.parametrize("nv,ne,seed", SHAPES)
def test_ids_fold_weights_and_prefix(nv, ne, seed):
    src, dst, w = synthetic_edges(nv, ne, seed, True)
    assert src.dtype == dst.dtype == np.int64 and w.dtype == np.float32
    assert src.min() >= 0 and dst.min() >= 0
    assert src.max() < nv and dst.max() < nv
    assert (w >= 1).all() and (w < 100).all()
    # the fold: raw ids lie below 2^scale < 2 nv and fold by one subtraction
    rs, rd, _ = raw_stream(nv, ne, seed)
    assert max(rs.max(), rd.max()) < (1 << scale_of(nv)) < 2 * nv
    folds = int(((rs >= nv) | (rd >= nv)).sum())
    assert (folds > 0) == (nv & (nv - 1) != 0)
    assert fold_ids(rs, nv).max() < nv
    # the stream of (nv, ne) is a prefix of that of (nv, 2 ne)
    s2, d2, w2 = synthetic_edges(nv, 2 * ne, seed, True)
    assert np.array_equal(s2[:ne], src) and np.array_equal(d2[:ne], dst)
    assert np.array_equal(w2[:ne], w)
    # unweighted: the same ids, no weights
    s3, d3, w3 = synthetic_edges(nv, ne, seed, False)
    assert w3 is None and np.array_equal(s3, src) and np.array_equal(d3, dst)
    # another seed is another stream
    s4, _, _ = synthetic_edges(nv, ne, seed + 1, False)
    assert not np.array_equal(s4, src)


def test_vectorised_model_equals_the_scalar_loop():
    cases = ((20000, 160000, 7, (0.57, 0.19, 0.19), True),
             (4096, 40000, 3, (0.57, 0.19, 0.19), True),
             (3000, 30000, 9, (0.45, 0.25, 0.15), True),
             (5000, 60000, 11, (0.57, 0.19, 0.19), False),
             (3, 50, 1, (0.57, 0.19, 0.19), True),
             (1, 50, 1, (0.57, 0.19, 0.19), True),
             (70000, 4000, (1 << 64) - 3, (0.57, 0.19, 0.19), True))
    for nv, ne, seed, abc, scr in cases:
        src, dst, w = synthetic_edges(nv, ne, seed, True, *abc, scramble=scr)
        idx = list(range(0, ne, max(1, ne // 300))) + [ne - 1]
        for i in idx:
            s, d, x = edge_int(i, nv, seed, *abc, scramble=scr)
            assert (int(src[i]), int(dst[i])) == (s, d), (nv, i)
            assert w[i] == weight_of_bits(np.array([x]))[0], (nv, i)


def test_rmat_skew_follows_abc():
    # the top bit of (s, d) is quadrant 0 with probability a, 3 with 1-a-b-c
    nv, ne = 4096, 40000
    rs, rd, _ = raw_stream(nv, ne, 3)
    top = (rs >> 11) * 2 + (rd >> 11)
    frac = np.bincount(top, minlength=4) / ne
    # 5 sigma of a binomial share over 40000 draws is below 0.0125
    assert np.allclose(frac, (0.57, 0.19, 0.19, 0.05), atol=0.0125), frac
    rs, rd, _ = raw_stream(nv, ne, 3, 0.45, 0.25, 0.15)
    top = (rs >> 11) * 2 + (rd >> 11)
    frac = np.bincount(top, minlength=4) / ne
    assert np.allclose(frac, (0.45, 0.25, 0.15, 0.15), atol=0.0125), frac


def test_weight_forms():
    # every fifth draw there is, and the last
    x = np.append(np.arange(0, 1 << 24, 5, dtype=np.int64), (1 << 24) - 1)
    fused, split = weight_of_bits(x), weight_of_bits(x, fused=False)
    assert fused.dtype == split.dtype == np.float32
    for w in (fused, split):
        assert w[0] == 1.0 and (w >= 1).all() and (w < 100).all()
        assert (np.diff(w) >= 0).all()
    assert fused[-1] < 100 and split[-1] < 100  # the largest draw
    # the fused form is the correctly rounded exact value
    exact = x.astype(np.float64) * 99.0 / 16777216.0 + 1.0  # exact in fp64
    assert np.array_equal(fused, exact.astype(np.float32))
    differ = int((fused != split).sum())
    assert 0.005 < differ / len(x) < 0.02, differ
    # never by more than one ulp
    assert (np.abs(fused.view(np.int32) - split.view(np.int32)) <= 1).all()
    # the figure quoted in the model's docstring
    _, _, a = synthetic_edges(20000, 160000, 7, True)
    _, _, b = synthetic_edges(20000, 160000, 7, True, fused=False)
    assert int((a != b).sum()) == 1633
