"""PageRank row scheduling on one GPU: isolated rows carried in closed form,
hub rows split into fixed segments, rows with out-edges only, hashmap
padding, and the BFS pull over buckets that hold no edgeless rows. Checked
against the NumPy oracles on graphs from load_edges."""
import numpy as np
import pytest

import grapehip
from oracles import bfs_oracle, pagerank_oracle, INT64_MAX

pytestmark = pytest.mark.gpu

RTOL, ATOL = 3e-5, 1e-12   # the project's PageRank tolerance
HUB_SEG = 4096             # arcs per hub work item (kHubSeg)


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29731, gpu=True)


def by_oid(res):
    return res["values"][np.argsort(res["oids"])]


def check_pr(vals, expect):
    assert abs(vals.sum() - 1.0) < 1e-5
    assert np.allclose(vals, expect, rtol=RTOL, atol=ATOL)


# -- 1. isolated rows -------------------------------------------------------

NV_ISO = 3001


@pytest.fixture(scope="module")
def iso_graph(eng):
    # edges only among 700 of 3001 ids; ids 0..9, 250..1199, 1500..2799 and
    # 2960..3000 are isolated (start, middle and end of the id range)
    rng = np.random.default_rng(5)
    live = np.r_[10:250, 1200:1500, 2800:2960]
    assert len(live) == 700
    src = live[rng.integers(0, len(live), 6000)]
    dst = live[rng.integers(0, len(live), 6000)]
    keep = src != dst
    src, dst = src[keep].astype(np.int64), dst[keep].astype(np.int64)
    g = eng.load_edges(src, dst, directed=False, num_vertices=NV_ISO)
    return g, src, dst


@pytest.mark.parametrize("iters", [1, 2, 10])
def test_isolated_rows(eng, iso_graph, iters):
    g, src, dst = iso_graph
    expect = pagerank_oracle(NV_ISO, src, dst, 0.85, iters, directed=False)
    # the captured iteration is replayed from the graph's second call on
    runs = [by_oid(eng.pagerank(g, 0.85, iters)) for _ in range(3)]
    for vals in runs:
        check_pr(vals, expect)
    for vals in runs[1:]:
        assert np.allclose(vals, runs[0], rtol=RTOL, atol=ATOL)
    touched = np.zeros(NV_ISO, bool)
    touched[src] = touched[dst] = True
    iso = runs[0][~touched]
    assert len(iso) >= NV_ISO - 700 and np.all(iso == iso[0])


def test_isolated_rows_l1_tolerance(eng, iso_graph):
    # tol > 0 stops on the L1 delta over ALL vertices, isolated included
    # (2301 of the 3001 terms here come from the closed form). The round
    # count is predicted by the oracle's iteration, stepped so that the delta
    # can be watched, with the engine's arithmetic: contributions rounded to
    # fp32, everything else fp64. That rounding puts a floor of a few 1e-10
    # under the delta, so the graph is one whose delta crosses tol with
    # room: 1.20e-9 in round 47, 7.5e-10 in round 48.
    g, src, dst = iso_graph
    tol, cap = 1e-9, 200
    s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])
    outdeg = np.bincount(s2, minlength=NV_ISO).astype(np.float64)
    r = np.full(NV_ISO, 1.0 / NV_ISO)
    rounds = 0
    while rounds < cap:
        c = np.where(outdeg > 0, r / np.maximum(outdeg, 1), 0.0)
        c = c.astype(np.float32).astype(np.float64)
        acc = np.bincount(d2, weights=c[s2], minlength=NV_ISO)
        nxt = 0.15 / NV_ISO + 0.85 * (acc + r[outdeg == 0].sum() / NV_ISO)
        l1 = np.abs(nxt - r).sum()
        r = nxt
        rounds += 1
        if l1 < tol:
            break
    assert rounds == 48
    expect = pagerank_oracle(NV_ISO, src, dst, 0.85, rounds, directed=False)
    assert np.allclose(r, expect, rtol=RTOL, atol=ATOL)
    res = eng.pagerank(g, 0.85, cap, tol=tol)
    print("l1 path: rounds gpu", res["rounds"], "oracle", rounds)
    assert res["rounds"] == rounds
    check_pr(by_oid(res), expect)


# -- 2. hub rows, 5. BFS pull from the hub ----------------------------------

NV_HUB = 40000
HUB_DEGS = [2 * 16384 + 37,   # large tier, 9 segments, ragged tail
            16384,            # exactly the tier boundary
            16383,            # stays in the mid tier
            HUB_SEG * 5 + 1]  # last segment holds one arc


@pytest.fixture(scope="module")
def hub_graph(eng):
    # hubs are ids 0..3 with distinct neighbours in [100, nv); the random
    # edges stay in [100, nv) too, so the hub degrees are exact and ids
    # 4..99 are isolated
    rng = np.random.default_rng(17)
    parts = []
    for h, d in enumerate(HUB_DEGS):
        nb = rng.choice(np.arange(100, NV_HUB), size=d, replace=False)
        parts.append(np.stack([np.full(d, h, np.int64), nb], 1))
    rnd = rng.integers(100, NV_HUB, size=(4000, 2))
    parts.append(rnd[rnd[:, 0] != rnd[:, 1]])
    e = np.concatenate(parts).astype(np.int64)
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    g = eng.load_edges(src, dst, directed=False, num_vertices=NV_HUB)
    return g, src, dst


def test_hub_rows(eng, hub_graph):
    g, src, dst = hub_graph
    expect = pagerank_oracle(NV_HUB, src, dst, 0.85, 10, directed=False)
    a = by_oid(eng.pagerank(g, 0.85, 10))
    b = by_oid(eng.pagerank(g, 0.85, 10))
    check_pr(a, expect)
    assert np.array_equal(a, b)   # no fp64 atomics on the hub sums


def test_bfs_pull_from_hub(eng, hub_graph):
    # the hub's 32805 out-edges exceed E/16, so level 0 already pulls
    g, src, dst = hub_graph
    vals = by_oid(eng.bfs(g, 0))
    assert np.array_equal(vals, bfs_oracle(NV_HUB, src, dst, 0,
                                           directed=False))
    assert np.all(vals[4:100] == INT64_MAX)


# -- 3. directed with an in-CSR ---------------------------------------------

def test_directed_in_csr(eng):
    # ids 0..499 only emit (in-degree 0), 1000..1499 only receive (dangling),
    # 1500..1999 have no edge at all
    rng = np.random.default_rng(29)
    nv = 2000
    src = rng.integers(0, 1000, 9000).astype(np.int64)
    dst = rng.integers(500, 1500, 9000).astype(np.int64)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    g = eng.load_edges(src, dst, directed=True, num_vertices=nv,
                       build_in_csr=True)
    expect = pagerank_oracle(nv, src, dst, 0.85, 10, directed=True)
    for _ in range(2):
        check_pr(by_oid(eng.pagerank(g, 0.85, 10)), expect)


# -- 4. sparse arbitrary oids (hashmap padding) -----------------------------

def test_sparse_oids_with_isolated(eng):
    rng = np.random.default_rng(73)
    nv = 3000
    oids = np.sort(rng.choice(10**9, size=nv, replace=False)).astype(np.int64)
    live = rng.choice(nv, size=1000, replace=False)
    si = live[rng.integers(0, len(live), 9000)]
    di = live[rng.integers(0, len(live), 9000)]
    keep = si != di
    si, di = si[keep], di[keep]
    g = eng.load_edges(oids[si], oids[di], directed=False, vertex_oids=oids)
    rp = eng.pagerank(g, 0.85, 10)
    assert len(rp["values"]) == nv
    assert abs(rp["values"].sum() - 1.0) < 1e-5
    expect = pagerank_oracle(nv, si, di, 0.85, 10, directed=False)
    got = dict(zip(rp["oids"].tolist(), rp["values"].tolist()))
    sample = np.arange(0, nv, 7)
    vals = np.array([got[int(oids[j])] for j in sample])
    assert np.allclose(vals, expect[sample], rtol=RTOL, atol=ATOL)
