"""Device fan-out (neighbourhood) sampler on one MI355X: the HIP path of
Engine.sample_neighbors against the NumPy oracle of test_fanout_oracle.py,
entry for entry.

Exact comparisons run on the simple graphs of test_gpu_sampler.py (unique
pairs, quarter weights: every fp32 row sum is exact in any order). Every
device call asserts that the `fanout_calls` counter of `_debug_sample` moved:
a silent host fallback fails.

`rounds` counts the levels that began with a live parent somewhere,
`traversed_edges` the samples drawn."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import grapehip
from test_fanout_oracle import (STRATEGIES, assert_same, fanout_oracle,
                                oracle_counts)
from test_gpu_kcore import pick_port
from test_gpu_sampler import (TIER_LENS, graph1_starts, simple_graph,
                              tier_graph)

REPO = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29761, gpu=True)


def device_fanout(eng, g, seeds, fanouts, **kw):
    """sample_neighbors on the device: the call counter must move."""
    before = eng._debug_sample()
    r = eng.sample_neighbors(g, np.asarray(seeds, dtype=np.int64), fanouts,
                             device=True, **kw)
    after = eng._debug_sample()
    assert after["fanout_calls"] == before["fanout_calls"] + 1
    assert after["calls"] == before["calls"]  # the walk counter stays
    for key in ("rounds", "seconds", "traversed_edges", "bytes_p2p",
                "bytes_coll"):
        assert key in r, key
    assert after["fanout_draws"] == r["traversed_edges"]
    return r


@functools.lru_cache(maxsize=None)
def graph1_oracle(directed, strategy):
    """The oracle's [3, 5, 2] table of the 2000-vertex graph, computed once."""
    src, dst, w = simple_graph(directed)
    return fanout_oracle(2000, src, dst, w, graph1_starts(), [3, 5, 2],
                         strategy, top_k=4, seed=7, directed=directed)


def assert_counts(r, want, ctx=None):
    rounds, draws = oracle_counts(want[1], want[2])
    assert r["rounds"] == rounds, ctx
    assert r["traversed_edges"] == draws, ctx


# --- 1. exact against the oracle --------------------------------------------

@pytest.mark.parametrize("directed", (True, False))
def test_exact_all_strategies(eng, directed):
    src, dst, w = simple_graph(directed)
    seeds = graph1_starts()
    g = eng.load_edges(src, dst, weights=w, directed=directed,
                       num_vertices=2000)
    for strategy in STRATEGIES:
        want = graph1_oracle(directed, strategy)
        leaves = want[1][:, want[2][-2]:]
        # 498 rows of 30 leaves; the oracle alone gives 14850 live leaves or
        # more in all six cases, so equality is not between empty tables
        assert leaves.shape == (498, 30) and (leaves >= 0).sum() > 12000
        r = device_fanout(eng, g, seeds, [3, 5, 2], strategy=strategy,
                          top_k=4, seed=7)
        assert_same(r, want, strategy)
        assert_counts(r, want, strategy)
        assert r["rounds"] == 3 and r["bytes_p2p"] == 0
        # fan-outs of 1 are walks
        r = device_fanout(eng, g, seeds, [1, 1, 1, 1], strategy=strategy,
                          top_k=4, seed=7)
        before = eng._debug_sample()["calls"]
        walk = eng.sample(g, seeds, hops=4, strategy=strategy, top_k=4,
                          seed=7, device=True)
        assert eng._debug_sample()["calls"] == before + 1
        assert np.array_equal(r["seed_ids"], walk["walk_ids"])
        assert np.array_equal(r["nodes"], walk["paths"])
        assert r["traversed_edges"] == walk["traversed_edges"]
        assert_same(r, fanout_oracle(2000, src, dst, w, seeds, [1] * 4,
                                     strategy, top_k=4, seed=7,
                                     directed=directed), strategy)
    # no levels: the seeds alone
    r = device_fanout(eng, g, seeds, [])
    assert_same(r, fanout_oracle(2000, src, dst, w, seeds, [],
                                 directed=directed))
    assert r["rounds"] == 0 and r["traversed_edges"] == 0


# --- 2. one parent wider than a wave ----------------------------------------

@pytest.mark.parametrize("fanouts", ([70], [2, 130]))
def test_parent_wider_than_a_wave(eng, fanouts):
    # 37 * 70 = 2590 items: no multiple of 256, siblings span two waves
    src, dst, w = simple_graph(True)
    seeds = graph1_starts()[:37]
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=2000)
    for strategy in STRATEGIES:
        want = fanout_oracle(2000, src, dst, w, seeds, fanouts, strategy,
                             top_k=4, seed=7)
        r = device_fanout(eng, g, seeds, fanouts, strategy=strategy, top_k=4,
                          seed=7)
        assert_same(r, want, (strategy, fanouts))
        assert_counts(r, want, (strategy, fanouts))


# --- 3. the row tiers of the index builds -----------------------------------

def test_row_tiers(eng):
    num_v, src, dst, w = tier_graph()
    seeds = np.arange(len(TIER_LENS))
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=num_v)
    cases = [("edge_weight", 4), ("random", 4), ("top_k", 1), ("top_k", 3),
             ("top_k", 32)]
    for strategy, k in cases:
        want = fanout_oracle(num_v, src, dst, w, seeds, [64], strategy,
                             top_k=k, seed=7)
        assert (want[1] >= 0).all()
        r = device_fanout(eng, g, seeds, [64], strategy=strategy, top_k=k,
                          seed=7)
        assert_same(r, want, (strategy, k))
    # the picks of the hub spread over its chunks
    assert len(np.unique(want[1][-1, 1:])) > 10


# --- 4. dead ends -----------------------------------------------------------

def test_dead_ends(eng):
    # 0 -> 1 -> 2 -> 3 -> 4 (a sink); 10 -> {11, 12} with weights 0
    src = np.array([0, 1, 2, 3, 10, 10], dtype=np.int64)
    dst = np.array([1, 2, 3, 4, 11, 12], dtype=np.int64)
    w = np.array([1, 1, 1, 1, 0, 0], dtype=np.float32)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=13)
    for strategy in STRATEGIES:
        r = device_fanout(eng, g, [0], [2] * 6, strategy=strategy)
        offs = r["level_offsets"]
        assert offs.tolist() == [0, 1, 3, 7, 15, 31, 63, 127]
        for h, v in enumerate((0, 1, 2, 3, 4)):
            assert (r["nodes"][0, offs[h]:offs[h + 1]] == v).all()
        assert (r["nodes"][0, offs[5]:] == -1).all()
        # level 5 still begins with live parents (the 4s) and draws nothing
        assert r["rounds"] == 5 and r["traversed_edges"] == 2 + 4 + 8 + 16
    r = device_fanout(eng, g, [10, 10, 4], [2, 2], strategy="edge_weight")
    assert r["nodes"].tolist() == [[10] + [-1] * 6] * 2 + [[4] + [-1] * 6]
    assert r["rounds"] == 1 and r["traversed_edges"] == 0
    r = device_fanout(eng, g, [10] * 4, [2, 2], strategy="random")
    assert set(r["nodes"][:, 1:3].ravel().tolist()) <= {11, 12}
    assert (r["nodes"][:, 3:] == -1).all() and r["rounds"] == 2
    assert_same(r, fanout_oracle(13, src, dst, w, [10] * 4, [2, 2], "random"))


# --- 5. device-only graph ---------------------------------------------------

def test_device_only_graph(eng):
    """No host fragment: the default runs on the device. The generator keeps
    its edges there, so a sample is checked through bfs: it lies at depth 1
    of its parent (a repeated vertex would be a self-loop, which bfs cannot
    show, and is not checked)."""
    g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7,
                           weighted=True)
    seeds = np.arange(0, 20000, 40, dtype=np.int64)
    parents = grapehip.fanout_parents([3, 3])
    checked = 0
    for strategy in STRATEGIES:
        before = eng._debug_sample()["fanout_calls"]
        r = eng.sample_neighbors(g, seeds, [3, 3], strategy=strategy, seed=5)
        assert eng._debug_sample()["fanout_calls"] == before + 1
        assert np.array_equal(r["seed_ids"], np.arange(500))
        assert r["nodes"].shape == (500, 13)
        assert np.array_equal(r["nodes"][:, 0], seeds)
        assert r["nodes"].max() < 20000 and r["nodes"].min() >= -1
        assert r["traversed_edges"] == int((r["nodes"][:, 1:] >= 0).sum()) > 0
        again = eng.sample_neighbors(g, seeds, [3, 3], strategy=strategy,
                                     seed=5)
        assert np.array_equal(again["nodes"], r["nodes"])
        other = eng.sample_neighbors(g, seeds, [3, 3], strategy=strategy,
                                     seed=6)
        assert not np.array_equal(other["nodes"], r["nodes"])
        full = r["nodes"][(r["nodes"] >= 0).all(axis=1)][:2]
        for row in full:
            for c in (1, 3, 4, 12):
                a, b = int(row[parents[c]]), int(row[c])
                if a == b:
                    continue
                d = eng.bfs(g, a)
                depth = np.asarray(d["values"])[np.argsort(d["oids"])]
                assert depth[b] == 1, (strategy, row, c)
                checked += 1
    assert checked >= 12


# --- 6. arbitrary oids ------------------------------------------------------

def test_arbitrary_oids(eng):
    """Hash vertex map: the device ids are renumbered, the rows come back in
    oids and every (parent, child) pair is an arc."""
    src, dst, w = simple_graph(False, num_v=500, arcs=6000, seed=251)
    rng = np.random.default_rng(252)
    oids = rng.choice(10 ** 12, size=500, replace=False).astype(np.int64)
    g = eng.load_edges(oids[src], oids[dst], weights=w, directed=False,
                       vertex_oids=oids, idxer="hashmap")
    arcs = set(zip(oids[src].tolist(), oids[dst].tolist()))
    arcs |= {(b, a) for a, b in arcs}
    seeds = np.concatenate([oids[:200], [5, -7]])
    parents = grapehip.fanout_parents([3, 2])
    for strategy in STRATEGIES:
        r = device_fanout(eng, g, seeds, [3, 2], strategy=strategy)
        assert np.array_equal(r["seed_ids"], np.arange(200))
        assert np.array_equal(r["nodes"][:, 0], oids[:200])
        live = 0
        for row in r["nodes"]:
            for c in range(1, 10):
                if row[c] >= 0:
                    assert (int(row[parents[c]]), int(row[c])) in arcs
                    live += 1
        # undirected: below a seed with an edge nothing is dead
        has_edge = np.bincount(np.concatenate([src, dst]),
                               minlength=500)[:200] > 0
        assert has_edge.sum() > 190
        assert live == r["traversed_edges"] == 9 * has_edge.sum()


# --- 7. index reuse ---------------------------------------------------------

def test_index_reuse(eng):
    src, dst, w = simple_graph(True, num_v=300, arcs=2000, seed=221)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    seeds = np.arange(64)
    eng._debug_sample(reset=True)
    device_fanout(eng, g, seeds, [2, 2], strategy="random")
    hook = eng._debug_sample()
    assert hook["cdf_builds"] == 0 and hook["topk_builds"] == 0
    # a cdf built by the walk serves the fan-out, and the other way round
    eng.sample(g, seeds, strategy="edge_weight", device=True)
    device_fanout(eng, g, seeds, [2, 2], strategy="edge_weight")
    device_fanout(eng, g, seeds, [2, 2], strategy="edge_weight", seed=8)
    assert eng._debug_sample()["cdf_builds"] == 1
    first = device_fanout(eng, g, seeds, [2, 2], strategy="top_k", top_k=3)
    eng.sample(g, seeds, strategy="top_k", top_k=3, device=True)
    again = device_fanout(eng, g, seeds, [2, 2], strategy="top_k", top_k=3)
    assert eng._debug_sample()["topk_builds"] == 1
    assert np.array_equal(first["nodes"], again["nodes"])
    r5 = device_fanout(eng, g, seeds, [2, 2], strategy="top_k", top_k=5)
    hook = eng._debug_sample()
    assert hook["topk_builds"] == 2 and hook["cdf_builds"] == 1
    assert hook["fanout_calls"] == 6 and hook["calls"] == 2
    assert_same(r5, fanout_oracle(300, src, dst, w, seeds, [2, 2], "top_k",
                                  top_k=5))
    g2 = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    device_fanout(eng, g2, seeds, [2, 2], strategy="edge_weight")
    assert eng._debug_sample()["cdf_builds"] == 2
    top_k_max = eng._debug_sample()["top_k_max"]
    with pytest.raises(RuntimeError, match="top_k = 33"):
        eng.sample_neighbors(g, seeds, [2], strategy="top_k",
                             top_k=top_k_max + 1, device=True)
    with pytest.raises(RuntimeError, match="top_k = 0"):
        eng.sample_neighbors(g, seeds, [2], strategy="top_k", top_k=0,
                             device=True)
    with pytest.raises(RuntimeError, match="kFanoutMaxEntries"):
        eng.sample_neighbors(g, seeds, [1000, 1000, 1000], device=True)
    # with a host fragment the default stays on the host
    before = eng._debug_sample()["fanout_calls"]
    r = eng.sample_neighbors(g, seeds, [2, 2])
    assert eng._debug_sample()["fanout_calls"] == before
    assert "traversed_edges" not in r
    assert_same(r, fanout_oracle(300, src, dst, w, seeds, [2, 2]))


# --- 8. worlds 2 and 4 over the TCP-staged data plane -----------------------

MULTI_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
import numpy as np
import grapehip
eng = grapehip.engine_from_env(gpu=True)
d = np.load(os.environ["GRAPEHIP_GRAPH"])
sl = slice(eng.rank, None, eng.world)
g = eng.load_edges(d["src"][sl], d["dst"][sl], weights=d["w"][sl],
                   directed=False, num_vertices=int(d["num_v"]))
out = {}
for strategy in ("random", "edge_weight", "top_k"):
    r = eng.sample_neighbors(g, d["seeds"], [3, 5, 2], strategy=strategy,
                             top_k=4, seed=7, device=True)
    out[strategy] = {"seed_ids": r["seed_ids"].tolist(),
                     "nodes": r["nodes"].tolist(),
                     "rounds": int(r["rounds"]),
                     "draws": int(r["traversed_edges"]),
                     "bytes_coll": int(r["bytes_coll"])}
out["fanout_calls"] = int(eng._debug_sample()["fanout_calls"])
path = os.path.join(os.environ["GRAPEHIP_OUT"],
                    "rank%s.json" % os.environ["RANK"])
json.dump(out, open(path, "w"))
'''


def run_world(world, outdir, port, graph_file):
    outdir.mkdir()
    procs = []
    for rank in range(world):
        # every rank on device 0: the ranks stage payloads through TCP
        env = dict(os.environ, GRAPEHIP_REPO=str(REPO),
                   GRAPEHIP_OUT=str(outdir), GRAPEHIP_GRAPH=str(graph_file),
                   RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world),
                   GRAPEHIP_DATAPLANE="tcp", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", MULTI_WORKER],
                                      env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=120)
            outs.append(o.decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    return [json.load(open(outdir / ("rank%d.json" % rank)))
            for rank in range(world)]


def test_worlds_match_the_oracle(tmp_path):
    src, dst, w = simple_graph(False)
    seeds = graph1_starts()
    graph_file = tmp_path / "graph.npz"
    np.savez(graph_file, src=src, dst=dst, w=w, seeds=seeds, num_v=2000)
    want = {s: graph1_oracle(False, s) for s in STRATEGIES}
    parents = grapehip.fanout_parents([3, 5, 2])
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        slice_ = (2000 + world - 1) // world
        for s in STRATEGIES:
            # at least a third of the oracle's samples leave their parent's
            # slice, so levels are completed by other ranks
            n = want[s][1]
            live = n[:, 1:] >= 0
            cross = live & (n[:, parents[1:]] // slice_ != n[:, 1:] // slice_)
            assert 3 * cross.sum() >= live.sum() > 4000, (world, s)
        ranks = run_world(world, tmp_path / ("w%d" % world), pick_port(),
                          graph_file)
        for d in ranks:
            assert d["fanout_calls"] == 3  # every result from the device
        for s in STRATEGIES:
            ids = np.concatenate([np.asarray(d[s]["seed_ids"], dtype=np.int64)
                                  for d in ranks])
            nodes = np.concatenate(
                [np.asarray(d[s]["nodes"], dtype=np.int64).reshape(-1, 49)
                 for d in ranks])
            # every seed on exactly one rank, with the oracle's row
            order = np.argsort(ids, kind="stable")
            assert np.array_equal(ids[order], want[s][0]), (world, s)
            assert np.array_equal(nodes[order], want[s][1]), (world, s)
            rounds, draws = oracle_counts(want[s][1], want[s][2])
            for rank, d in enumerate(ranks):
                own = seeds[np.asarray(d[s]["seed_ids"], dtype=np.int64)]
                assert ((own // slice_) == rank).all(), (world, s, rank)
                assert d[s]["rounds"] == rounds == 3
                assert d[s]["draws"] == draws
                assert d[s]["bytes_coll"] > 0, (world, s, rank)
