"""GPU CDLP on a graph built to put a row on every tier bound and to show
that rows of every tier are recomputed once the dirty-row gate is on: rows
whose stored degree is each tier's upper bound and the next value up plus one
clear hub, all hanging on planted communities that let the labels settle."""
import functools

import numpy as np
import pytest

from oracles import cdlp_oracle_fast

ITERS = 10
# tiny, small, wave and mid tier bounds, each with the next value up, and a hub
DEGREES = [16, 17, 64, 65, 512, 513, 4096, 4097, 12000]
N_SPECIAL = len(DEGREES)
N_COMMUNITIES = 120
N_ISOLATED = 50


def build_edges():
    """Returns (src, dst, num_v). Vertices 0..8 are the special rows, then
    the communities (the pool), then the isolated vertices."""
    rng = np.random.default_rng(73)
    src, dst = [], []
    pool_lo = pool_hi = N_SPECIAL
    for _ in range(N_COMMUNITIES):
        # the communities of test_gpu_schedulers.sched_graph
        n = int(rng.integers(100, 501))
        ids = np.arange(pool_hi, pool_hi + n, dtype=np.int64)
        pool_hi += n
        a = rng.integers(0, n, 10 * n)
        b = rng.integers(0, n, 10 * n)
        keep = a != b
        src.append(ids[a[keep]])
        dst.append(ids[b[keep]])
    for v, deg in enumerate(DEGREES):
        # two thirds of the arcs to distinct pool vertices, the rest repeat
        # them: counts above 1, and ties
        distinct = rng.choice(np.arange(pool_lo, pool_hi), 2 * deg // 3,
                              replace=False)
        others = np.concatenate([distinct,
                                 rng.choice(distinct, deg - len(distinct))])
        # alternate the stored direction, so the directed run has the row's
        # arcs in both the out- and the in-CSR
        me = np.full(deg, v, dtype=np.int64)
        flip = np.arange(deg) % 2 == 1
        src.append(np.where(flip, others, me))
        dst.append(np.where(flip, me, others))
    return np.concatenate(src), np.concatenate(dst), pool_hi + N_ISOLATED


@functools.lru_cache(maxsize=None)
def expected():
    """The graph and its oracle labels, computed once for the module; the
    oracle reads the arcs both ways, so one result serves both loads."""
    src, dst, num_v = build_edges()
    labels, changed = cdlp_oracle_fast(num_v, src, dst, ITERS,
                                       return_changed=True)
    return src, dst, num_v, labels, changed


def test_graph_meets_the_conditions():
    # what the GPU cases rely on, from the oracle alone
    src, dst, num_v, _, changed = expected()
    assert 30000 < num_v < 50000 and 300000 < len(src) < 500000
    # undirected storage holds both orientations, directed tiers by out + in
    deg = np.bincount(src, minlength=num_v) + np.bincount(dst,
                                                          minlength=num_v)
    assert deg[:N_SPECIAL].tolist() == DEGREES
    assert deg[N_SPECIAL:].max() <= 64
    assert (deg == 0).sum() == N_ISOLATED
    # the engine recomputes only dirty rows in iteration j (from 0) when
    # fewer than 1/8 of the labels changed in iteration j - 1
    gate = num_v // 8
    gated = [j for j in range(1, ITERS) if 0 < changed[j - 1] < gate]
    assert gated, changed
    j = gated[0]
    # labels that changed in iteration j - 1 make their neighbours dirty in j
    before = cdlp_oracle_fast(num_v, src, dst, j - 1)
    after = cdlp_oracle_fast(num_v, src, dst, j)
    moved = before != after
    assert moved.sum() == changed[j - 1]
    for v in range(N_SPECIAL):
        nbrs = np.concatenate([dst[src == v], src[dst == v]])
        assert moved[nbrs].any(), v


@pytest.fixture(scope="module")
def eng():
    import grapehip
    return grapehip.Engine(rank=0, world=1, master_port=29723, gpu=True)


def by_oid(res):
    return res["values"][np.argsort(res["oids"])]


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_cdlp_every_tier_bound(eng, directed):
    src, dst, num_v, labels, _ = expected()
    g = eng.load_edges(src, dst, directed=directed, num_vertices=num_v,
                       build_in_csr=directed)
    assert np.array_equal(by_oid(eng.cdlp(g, ITERS)), labels)


@pytest.mark.gpu
@pytest.mark.parametrize("directed", [False, True])
def test_gpu_cdlp_no_edges(eng, directed):
    none = np.zeros(0, dtype=np.int64)
    g = eng.load_edges(none, none, directed=directed, num_vertices=100,
                       build_in_csr=directed)
    res = eng.cdlp(g, ITERS)
    assert len(res["values"]) == 100
    assert np.array_equal(res["values"], res["oids"])
