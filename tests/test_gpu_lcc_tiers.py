"""GPU LCC on a graph built to reach every dedup tier: rows whose stored
degree sits on each tier bound and one above it, rows with duplicate arcs and
a self loop in each tier, and adjacent rows of equal distinct degree."""
import numpy as np
import pytest

import grapehip
from oracles import lcc_oracle

pytestmark = pytest.mark.gpu

NV = 30000
# kTierSmallDeg, kTierWaveDeg, kTierMidDeg, each with the next value up
BOUNDS = [64, 65, 512, 513, 4096, 4097]
# (stored degree, distinct filler values) of the duplicate-arc rows, one per
# tier: small, wave, mid, large
DEDUP = [(40, 12), (300, 100), (2000, 700), (6000, 2500)]
N_SPECIAL = len(BOUNDS) + len(DEDUP)
TIE_P, TIE_Q = NV - 2, NV - 1       # adjacent, equal distinct degree
POOL_LO, POOL_HI = N_SPECIAL, NV - 2  # everything else


def build_edges():
    rng = np.random.default_rng(71)
    edges = []

    def arcs(v, others):
        # alternate the stored direction, so the directed run has the row's
        # arcs in both the out- and the in-CSR
        for k, o in enumerate(others):
            edges.append((v, o) if k % 2 == 0 else (o, v))

    # the special rows form a clique: every one of them closes triangles
    for a in range(N_SPECIAL):
        for b in range(a + 1, N_SPECIAL):
            edges.append((a, b) if (a + b) % 2 == 0 else (b, a))
    core = N_SPECIAL - 1
    for v, deg in enumerate(BOUNDS):
        arcs(v, rng.choice(np.arange(POOL_LO, POOL_HI), deg - core,
                           replace=False))
    for i, (deg, distinct) in enumerate(DEDUP):
        v = len(BOUNDS) + i
        vals = rng.choice(np.arange(POOL_LO, POOL_HI), distinct,
                          replace=False)
        edges.append((v, v))  # self loop: 2 stored entries, no neighbor
        fill = deg - core - 2
        # every value once, the rest repeats
        arcs(v, np.concatenate([vals, rng.choice(vals, fill - distinct)]))
    # tie pair: adjacent, both with the same five further neighbors
    edges.append((TIE_P, TIE_Q))
    for x in rng.choice(np.arange(POOL_LO, POOL_HI), 5, replace=False):
        edges.append((TIE_P, x))
        edges.append((x, TIE_Q))
    # background among the pool vertices (self loops and duplicates stay in)
    bg = rng.integers(POOL_LO, POOL_HI, size=(40000, 2))
    e = np.concatenate([np.asarray(edges, dtype=np.int64), bg])
    e = e[rng.permutation(len(e))]
    return np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])


def stored_degree(src, dst):
    # undirected storage holds both orientations (a self loop twice);
    # directed tiers by out + in: the same count either way
    return np.bincount(src, minlength=NV) + np.bincount(dst, minlength=NV)


def distinct_degree(src, dst, v):
    nb = set(dst[src == v]) | set(src[dst == v])
    nb.discard(v)
    return len(nb)


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29719, gpu=True)


def checked_edges():
    src, dst = build_edges()
    deg = stored_degree(src, dst)
    assert list(deg[:len(BOUNDS)]) == BOUNDS
    assert not np.any((src == dst) & (src < len(BOUNDS)))
    uppers = [64, 512, 4096, 1 << 31]
    lowers = [0, 64, 512, 4096]
    for i, (d, _) in enumerate(DEDUP):
        v = len(BOUNDS) + i
        assert deg[v] == d and lowers[i] < d <= uppers[i]
        assert distinct_degree(src, dst, v) < d - 2
        assert np.any((src == v) & (dst == v))
    assert distinct_degree(src, dst, TIE_P) == distinct_degree(src, dst,
                                                               TIE_Q) == 6
    return src, dst


@pytest.fixture(scope="module")
def graph():
    return checked_edges()


def by_oid(res):
    return res["values"][np.argsort(res["oids"])]


@pytest.mark.parametrize("directed", [False, True])
def test_gpu_lcc_every_tier(eng, graph, directed):
    src, dst = graph
    expect = lcc_oracle(NV, src, dst, directed=directed)
    assert np.all(expect[:N_SPECIAL] > 0)
    assert expect[TIE_P] > 0 and expect[TIE_Q] > 0
    g = eng.load_edges(src, dst, directed=directed, num_vertices=NV,
                       build_in_csr=directed)
    assert np.allclose(by_oid(eng.lcc(g)), expect, rtol=1e-12)


@pytest.mark.parametrize("directed", [False, True])
def test_gpu_lcc_no_edges(eng, directed):
    none = np.zeros(0, dtype=np.int64)
    g = eng.load_edges(none, none, directed=directed, num_vertices=100,
                       build_in_csr=directed)
    vals = by_oid(eng.lcc(g))
    assert len(vals) == 100 and not np.any(vals)
