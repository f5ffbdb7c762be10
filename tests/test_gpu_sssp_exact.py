"""GPU SSSP held to bit equality with fp32 Dijkstra (sssp_oracle_f32).

SsspOp computes dist[u] + w in fp32 (one add, nothing to contract), lowers
dist[d] with an atomic min and re-queues every vertex it lowers. fp32
addition is monotone, so any relaxation order run to convergence gives the
minimum over paths of the left-to-right fp32 sum: what Dijkstra in fp32
arithmetic returns (tests/test_oracle_sssp_f32.py checks that claim on the
CPU). So the scheduler, the bucket width delta and the order in which the
segmented sort leaves a row's arcs must not change one bit of the result."""
import numpy as np
import pytest

import grapehip
from oracles import sssp_oracle_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29741, gpu=True)


def by_oid(res):
    return np.asarray(res["values"])[np.argsort(res["oids"])]


def assert_exact(got, exp):
    unreached = exp > 1e300
    assert np.array_equal(got > 1e300, unreached)
    assert np.array_equal(got[~unreached].astype(np.float32),
                          exp[~unreached].astype(np.float32))


def weights(rng, n):
    return (rng.random(n, dtype=np.float32) * 9 + 1).astype(np.float32)


# -- 1. mixed random ---------------------------------------------------------

N_ISOLATED = 50   # the last ids: no arc at all
N_SINKS = 30      # the ids before them: never a source of an arc


def mixed_graph(num_v, num_e, seed):
    """Random multigraph. Weights in [1,10), 5% of them exactly 0; 200
    parallel pairs (same src and dst) with the lighter arc second in input
    order; 20 self-loops; 30 vertices that are only ever a dst; 50 vertices
    without arcs."""
    rng = np.random.default_rng(seed)
    n_src = num_v - N_ISOLATED - N_SINKS
    n_dst = num_v - N_ISOLATED
    src = rng.integers(0, n_src, num_e).astype(np.int64)
    dst = rng.integers(0, n_dst, num_e).astype(np.int64)
    w = weights(rng, num_e)
    w[rng.random(num_e) < 0.05] = 0.0
    ps = rng.integers(0, n_src, 200).astype(np.int64)
    pd = rng.integers(0, n_dst, 200).astype(np.int64)
    heavy = (rng.random(200, dtype=np.float32) * 4 + 5).astype(np.float32)
    light = (rng.random(200, dtype=np.float32) * 3 + 1).astype(np.float32)
    lv = rng.choice(n_src, 20, replace=False).astype(np.int64)
    src = np.concatenate([src, np.stack([ps, ps], 1).ravel(), lv])
    dst = np.concatenate([dst, np.stack([pd, pd], 1).ravel(), lv])
    w = np.concatenate([w, np.stack([heavy, light], 1).ravel(),
                        weights(rng, 20)])
    assert (w == 0).sum() > num_e // 40
    return src, dst, w


DIRECTED = (3000, 20000, 31)
UNDIRECTED = (2000, 12000, 32)


@pytest.fixture(scope="module")
def directed_graph(eng):
    num_v = DIRECTED[0]
    src, dst, w = mixed_graph(*DIRECTED)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=num_v)
    return g, num_v, src, dst, w


@pytest.fixture(scope="module")
def undirected_graph(eng):
    num_v = UNDIRECTED[0]
    src, dst, w = mixed_graph(*UNDIRECTED)
    g = eng.load_edges(src, dst, weights=w, directed=False,
                       num_vertices=num_v)
    return g, num_v, src, dst, w


def test_mixed_directed(eng, directed_graph):
    g, num_v, src, dst, w = directed_graph
    sink = num_v - N_ISOLATED - 1
    assert (dst == sink).any() and not (src == sink).any()
    for source in (int(src[0]), num_v - 1, sink):
        exp = sssp_oracle_f32(num_v, src, dst, w, source, directed=True)
        assert_exact(by_oid(eng.sssp(g, source)), exp)
        if source != int(src[0]):
            # only the source is reached, at 0
            assert exp[source] == 0.0 and (exp < 1e300).sum() == 1
        else:
            assert (exp < 1e300).sum() > num_v // 2


def test_mixed_undirected(eng, undirected_graph):
    g, num_v, src, dst, w = undirected_graph
    for source in (int(src[0]), num_v - 1):
        exp = sssp_oracle_f32(num_v, src, dst, w, source, directed=False)
        assert_exact(by_oid(eng.sssp(g, source)), exp)
        if source == num_v - 1:
            assert exp[source] == 0.0 and (exp < 1e300).sum() == 1
        else:
            assert (exp < 1e300).sum() > num_v // 2


# -- 2. delta sweep ----------------------------------------------------------

def test_delta_sweep(eng, undirected_graph):
    # -1: the automatic width. 0.5: below every positive weight, so every
    # relaxation over a positive arc lands in the far queue and each bucket
    # is a priority advance with a repartition. 16 x mean: the plateau.
    # 1e30: everything is near, plain Bellman-Ford rounds.
    g, num_v, src, dst, w = undirected_graph
    source = int(src[0])
    exp = sssp_oracle_f32(num_v, src, dst, w, source, directed=False)
    assert w[w > 0].min() > 0.5
    # the advance loop walks the buckets one host sync at a time: at most
    # 512 of them at the narrowest width (a condition on the graph, checked
    # before the GPU is touched)
    assert exp[exp < 1e300].max() / 0.5 <= 512
    for delta in (-1.0, 0.5, 16 * float(w.mean()), 1e30):
        assert_exact(by_oid(eng.sssp(g, source, delta=delta)), exp)


# -- 3. weighted hub rows and sort tiers ------------------------------------

HUB_DEGS = (1, 2, 3, 4096, 4097, 16383, 16384, 2 * 16384 + 37)
N_REST = 3000
N_DUP = 500


def hub_graph():
    """Undirected. Hub i has exactly HUB_DEGS[i] stored arcs: to the first
    HUB_DEGS[i] ids of a leaf range that only hubs touch, so no row but the
    largest holds a neighbour twice. The largest hub reaches 500 of its
    leaves twice, with different weights. 4000 random weighted edges join
    the N_REST vertices between hubs and leaves; they hang on the hubs by one
    edge from a leaf. Row sizes sit on both sides of the LDS sort's 4096 and
    of 16384; the largest row is padded to 65536 by the global sort and is a
    frontier entry of 32,805 arcs."""
    rng = np.random.default_rng(33)
    n_hubs = len(HUB_DEGS)
    rest0 = n_hubs
    leaf0 = rest0 + N_REST
    n_leaves = HUB_DEGS[-1] - N_DUP
    num_v = leaf0 + n_leaves
    src, dst = [], []
    for i, deg in enumerate(HUB_DEGS):
        leaves = np.arange(leaf0, leaf0 + min(deg, n_leaves), dtype=np.int64)
        if i == n_hubs - 1:
            leaves = np.concatenate([leaves, leaves[100:100 + N_DUP]])
        assert len(leaves) == deg
        src.append(np.full(deg, i, dtype=np.int64))
        dst.append(leaves)
    rs = rng.integers(rest0, rest0 + N_REST, 4000).astype(np.int64)
    rd = rng.integers(rest0, rest0 + N_REST, 4000).astype(np.int64)
    # the last leaf (a neighbour of the largest hub alone) ties in the rest
    src = np.concatenate(src + [rs, [num_v - 1]])
    dst = np.concatenate(dst + [rd, [rs[0]]])
    w = weights(rng, len(src))
    return src, dst, w, num_v, leaf0


def test_hub_rows_and_sort_tiers(eng):
    src, dst, w, num_v, leaf0 = hub_graph()
    assert 35000 <= num_v <= 45000
    n_hubs = len(HUB_DEGS)
    deg = np.bincount(src, minlength=num_v) + np.bincount(dst,
                                                          minlength=num_v)
    assert tuple(deg[:n_hubs]) == HUB_DEGS
    g = eng.load_edges(src, dst, weights=w, directed=False,
                       num_vertices=num_v)
    # the largest hub, a leaf it reaches twice, a vertex of the random part
    for source in (n_hubs - 1, leaf0 + 100, int(src[-2])):
        exp = sssp_oracle_f32(num_v, src, dst, w, source, directed=False)
        assert (exp < 1e300).sum() > num_v - N_REST
        assert_exact(by_oid(eng.sssp(g, source)), exp)


# -- 4. sparse arbitrary oids -----------------------------------------------

def test_sparse_oids(eng):
    rng = np.random.default_rng(34)
    num_v = 2000
    si = rng.integers(0, num_v, 12000).astype(np.int64)
    di = rng.integers(0, num_v, 12000).astype(np.int64)
    w = weights(rng, 12000)
    oids = rng.choice(10**12, size=num_v, replace=False).astype(np.int64)
    g = eng.load_edges(oids[si], oids[di], weights=w, directed=False,
                       vertex_oids=oids, idxer="hashmap")
    exp = sssp_oracle_f32(num_v, si, di, w, 5, directed=False)
    r = eng.sssp(g, int(oids[5]))
    assert np.array_equal(np.sort(r["oids"]), np.sort(oids))
    got = dict(zip(r["oids"].tolist(), np.asarray(r["values"]).tolist()))
    assert_exact(np.array([got[int(o)] for o in oids]), exp)
    assert exp[5] == 0.0 and (exp < 1e300).sum() > num_v // 2
