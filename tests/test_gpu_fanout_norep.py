"""Device fan-out sampler without replacement on one MI355X: the HIP path of
Engine.sample_neighbors(replace=False) against the NumPy oracle of
test_fanout_norep_oracle.py, entry for entry.

The level kernel gives one group of W lanes to a parent, W the smallest
power of two >= f, so the cases walk the group shapes: f = 1, 2, a group with
an idle lane (3), 5, more than half a wave (33), 63 and 64, levels whose
parents were written by the device and are partly dead, and a seed count
that leaves the last wave with a partial set of groups."""
import functools
import json
import os
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import grapehip
from test_fanout_norep_oracle import fanout_oracle_norep
from test_fanout_oracle import fanout_oracle
from test_gpu_fanout import assert_counts, assert_same, device_fanout
from test_gpu_kcore import pick_port
from test_gpu_sampler import (TIER_LENS, graph1_starts, quarter_weights,
                              simple_graph, tier_graph)
from test_sampler_draw_oracle import build_rows

REPO = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29781, gpu=True)


# --- 1. the group shapes, on rows of every length ---------------------------

@functools.lru_cache(maxsize=None)
def tiers():
    """tier_graph() and one more row, of 6 arcs (vertex len(TIER_LENS)), so
    that deg == f + 1 occurs for f = 5 too. 37 seeds: every row, sinks, ids
    that are no vertex, the hub and short rows again."""
    num_v, src, dst, w = tier_graph()
    v = len(TIER_LENS)
    src = np.concatenate([src, np.full(6, v, dtype=np.int64)])
    dst = np.concatenate([dst, np.arange(200, 206, dtype=np.int64)])
    w = np.concatenate([w, quarter_weights(np.random.default_rng(212), 6)])
    seeds = np.concatenate([np.arange(v + 1), [300, num_v + 7, -1, 301],
                            [v - 1, v - 1, 0, 1, 2, 3, 4, 8, 9, 12, 13, 14,
                             16]]).astype(np.int64)
    assert len(seeds) == 37
    return num_v, src, dst, w, seeds


@pytest.fixture(scope="module")
def tier_dev(eng):
    num_v, src, dst, w, _ = tiers()
    return (eng.load_edges(src, dst, weights=w, directed=True,
                           num_vertices=num_v),
            eng.load_edges(src, dst, directed=True, num_vertices=num_v))


@pytest.mark.parametrize("f", (1, 2, 3, 5, 33, 63, 64))
def test_group_shapes(eng, tier_dev, f):
    num_v, src, dst, w, seeds = tiers()
    deg = np.bincount(src, minlength=num_v)
    live = seeds[(seeds >= 0) & (seeds < num_v)]
    pdeg = set(deg[live].tolist())
    # the parents of the oracle: shorter than, as long as, one longer than
    # the fan-out, and a hub
    assert min(pdeg) < f and {f, f + 1} <= pdeg and max(pdeg) >= 4096
    for weights, g in zip((w, None), tier_dev):
        for strategy, k in (("random", 4), ("top_k", 4), ("top_k", 32)):
            want = fanout_oracle_norep(num_v, src, dst, weights, seeds, [f],
                                       strategy, top_k=k, seed=7)
            r = device_fanout(eng, g, seeds, [f], strategy=strategy, top_k=k,
                              seed=7, replace=False)
            ctx = (f, strategy, k, weights is not None)
            assert_same(r, want, ctx)
            assert_counts(r, want, ctx)
            m = deg[live] if strategy == "random" else np.minimum(deg[live], k)
            assert r["traversed_edges"] == np.minimum(m, f).sum()


def test_top_k_through_the_index(eng, tier_dev):
    num_v, src, dst, w, seeds = tiers()
    off, adj, aw = build_rows(num_v, src, dst, w)
    g = tier_dev[0]
    for k in (32, 3):
        want = fanout_oracle_norep(num_v, src, dst, w, seeds, [8], "top_k",
                                   top_k=k, seed=7)
        r = device_fanout(eng, g, seeds, [8], strategy="top_k", top_k=k,
                          seed=7, replace=False)
        assert_same(r, want, k)
        # the hub (deg 5000 > k): 8 distinct arcs of its 32 heaviest, or the
        # ranked three
        hub = len(TIER_LENS) - 1
        b, e = int(off[hub]), int(off[hub + 1])
        order = sorted(range(e - b), key=lambda s: (-float(aw[b + s]), s))
        heavy = [int(adj[b + s]) for s in order[:k]]
        kids = [x for x in r["nodes"][hub, 1:].tolist() if x >= 0]
        assert len(kids) == min(k, 8) == len(set(kids))
        assert set(kids) <= set(heavy)
        if k == 3:
            assert kids == heavy
    assert eng._debug_sample()["topk_builds"] >= 2


# --- 2. levels written by the device ----------------------------------------

@functools.lru_cache(maxsize=None)
def graph1_norep_oracle(directed, weighted, strategy):
    """The oracle's [3, 5] table of the 2000-vertex graph, computed once."""
    src, dst, w = simple_graph(directed)
    return fanout_oracle_norep(2000, src, dst, w if weighted else None,
                               graph1_starts(), [3, 5], strategy, top_k=4,
                               seed=7, directed=directed)


@pytest.mark.parametrize("weighted", (True, False))
@pytest.mark.parametrize("directed", (True, False))
def test_exact_two_levels(eng, directed, weighted):
    src, dst, w = simple_graph(directed)
    if not weighted:
        w = None
    seeds = graph1_starts()
    g = eng.load_edges(src, dst, weights=w, directed=directed,
                       num_vertices=2000)
    strategies = ("random", "top_k") + (() if weighted else ("edge_weight",))
    for strategy in strategies:
        want = graph1_norep_oracle(directed, weighted, strategy)
        leaves = want[1][:, want[2][-2]:]
        # dead parents (-1 after a short row) share waves with live ones
        mid = want[1][:, 1:4]
        assert leaves.shape == (498, 15) and (leaves >= 0).sum() > 3000
        assert (mid < 0).any() and (mid >= 0).sum() > 1000
        r = device_fanout(eng, g, seeds, [3, 5], strategy=strategy, top_k=4,
                          seed=7, replace=False)
        assert_same(r, want, strategy)
        assert_counts(r, want, strategy)
        assert r["rounds"] == 2 and r["bytes_p2p"] == 0
        with_r = device_fanout(eng, g, seeds, [3, 5], strategy=strategy,
                               top_k=4, seed=7)
        assert sorted(with_r) == sorted(r)  # the same keys
        assert not np.array_equal(with_r["nodes"], r["nodes"])
        # 37 seeds: the last wave holds a partial set of groups
        for fanouts in ([5, 3], [64, 2]):
            want = fanout_oracle_norep(2000, src, dst, w, seeds[:37], fanouts,
                                       strategy, top_k=4, seed=7,
                                       directed=directed)
            r = device_fanout(eng, g, seeds[:37], fanouts, strategy=strategy,
                              top_k=4, seed=7, replace=False)
            assert_same(r, want, (strategy, fanouts))
            assert_counts(r, want, (strategy, fanouts))
    # no levels: the seeds alone
    r = device_fanout(eng, g, seeds, [], replace=False)
    assert_same(r, fanout_oracle_norep(2000, src, dst, w, seeds, [],
                                       directed=directed))
    assert r["rounds"] == 0 and r["traversed_edges"] == 0


# --- 3. unit fan-outs -------------------------------------------------------

def test_unit_fanouts_are_walks(eng):
    src, dst, w = simple_graph(False)
    seeds = graph1_starts()
    g = eng.load_edges(src, dst, weights=w, directed=False, num_vertices=2000)
    for strategy in ("random", "top_k"):
        a = device_fanout(eng, g, seeds, [1] * 4, strategy=strategy, top_k=4,
                          seed=7, replace=False)
        b = device_fanout(eng, g, seeds, [1] * 4, strategy=strategy, top_k=4,
                          seed=7, replace=True)
        walk = eng.sample(g, seeds, hops=4, strategy=strategy, top_k=4,
                          seed=7, device=True)
        assert np.array_equal(a["nodes"], b["nodes"])
        assert np.array_equal(a["seed_ids"], walk["walk_ids"])
        assert np.array_equal(a["nodes"], walk["paths"])
        assert a["traversed_edges"] == walk["traversed_edges"] > 1500
        assert_same(a, fanout_oracle(2000, src, dst, w, seeds, [1] * 4,
                                     strategy, top_k=4, seed=7,
                                     directed=False), strategy)


# --- 4. device-only graph ---------------------------------------------------

def test_device_only_graph(eng):
    """No host fragment, hub-renumbered, parallel arcs possible: the live
    children of every parent are a sub-multiset of its stored row, min(deg,
    f) of them."""
    g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7,
                           weighted=True)
    c = eng._debug_csr(g)
    off = c["off"].astype(np.int64)
    dst = c["dst"].astype(np.int64)
    if c["new_of_old"] is None:
        new_of_old = old_of_new = np.arange(20000)
    else:
        new_of_old = c["new_of_old"].astype(np.int64)
        old_of_new = c["old_of_new"].astype(np.int64)

    def row_of(v):
        n = new_of_old[v]
        return old_of_new[dst[off[n]:off[n + 1]]].tolist()

    seeds = np.arange(0, 20000, 40, dtype=np.int64)
    fanouts = [6, 3]
    parents = grapehip.fanout_parents(fanouts)
    before = eng._debug_sample()["fanout_calls"]
    r = eng.sample_neighbors(g, seeds, fanouts, seed=5, replace=False)
    assert eng._debug_sample()["fanout_calls"] == before + 1
    nodes = r["nodes"]
    assert nodes.shape == (500, 25)
    assert np.array_equal(nodes[:, 0], seeds)
    assert r["traversed_edges"] == int((nodes[:, 1:] >= 0).sum()) > 1000
    firsts = [(1, 6)] + [(7 + 3 * j, 3) for j in range(6)]
    short = long = 0
    for row in nodes.tolist():
        for first, f in firsts:
            parent = row[parents[first]]
            kids = row[first:first + f]
            live = [k for k in kids if k >= 0]
            assert kids == live + [-1] * (f - len(live)), row
            if parent < 0:
                assert not live, row
                continue
            stored = row_of(parent)
            assert len(live) == min(len(stored), f), (row, first)
            assert not Counter(live) - Counter(stored), (row, first)
            short += 0 < len(stored) <= f
            long += len(stored) > f
    assert short > 20 and long > 20
    again = eng.sample_neighbors(g, seeds, fanouts, seed=5, replace=False)
    assert np.array_equal(again["nodes"], nodes)
    # top_k through the index of a renumbered graph: within the k heaviest
    r = eng.sample_neighbors(g, seeds, [4], strategy="top_k", top_k=8,
                             seed=5, replace=False)
    assert (r["nodes"][:, 1:] >= 0).sum() > 500
    w = c["w"]
    for row in r["nodes"][:100].tolist():
        n = new_of_old[row[0]]
        b, e = off[n], off[n + 1]
        order = sorted(range(e - b), key=lambda s: (-float(w[b + s]), s))
        heavy = Counter(old_of_new[dst[b:e][order[:8]]].tolist())
        live = [k for k in row[1:] if k >= 0]
        assert len(live) == min(e - b, 4) and not Counter(live) - heavy, row


# --- 5. errors --------------------------------------------------------------

def test_errors(eng):
    src, dst, w = simple_graph(True, num_v=300, arcs=2000, seed=221)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    seeds = np.arange(64)
    before = eng._debug_sample()["fanout_calls"]
    with pytest.raises(RuntimeError, match="fanout = 70 is above 64") as err:
        eng.sample_neighbors(g, seeds, [2, 70], device=True, replace=False)
    assert "kFanoutNoReplaceMax" in str(err.value)
    with pytest.raises(RuntimeError, match="edge_weight") as err:
        eng.sample_neighbors(g, seeds, [2], strategy="edge_weight",
                             device=True, replace=False)
    assert "replace=False" in str(err.value)
    with pytest.raises(RuntimeError, match="top_k = 33"):
        eng.sample_neighbors(g, seeds, [2], strategy="top_k", top_k=33,
                             device=True, replace=False)
    assert eng._debug_sample()["fanout_calls"] == before
    # with replacement the wide fan-out still runs
    want = fanout_oracle(300, src, dst, w, seeds, [2, 70])
    assert_same(device_fanout(eng, g, seeds, [2, 70], replace=True), want)
    # and the host path takes it without replacement
    r = eng.sample_neighbors(g, seeds, [2, 70], device=False, replace=False)
    assert_same(r, fanout_oracle_norep(300, src, dst, w, seeds, [2, 70]))


# --- 6. worlds 2 and 4 over the TCP-staged data plane -----------------------

NOREP_MULTI_WORKER = r'''
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
for strategy in ("random", "top_k"):
    r = eng.sample_neighbors(g, d["seeds"], [3, 5], strategy=strategy,
                             top_k=4, seed=7, device=True, replace=False)
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
        procs.append(subprocess.Popen(
            [sys.executable, "-c", NOREP_MULTI_WORKER], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
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
    want = {s: graph1_norep_oracle(False, True, s)
            for s in ("random", "top_k")}
    parents = grapehip.fanout_parents([3, 5])
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        slice_ = (2000 + world - 1) // world
        for s, (_, n, offs) in want.items():
            # many samples leave their parent's slice, so levels are
            # completed by other ranks
            live = n[:, 1:] >= 0
            cross = live & (n[:, parents[1:]] // slice_ != n[:, 1:] // slice_)
            assert 3 * cross.sum() >= live.sum() > 4000, (world, s)
        ranks = run_world(world, tmp_path / ("w%d" % world), pick_port(),
                          graph_file)
        for d in ranks:
            assert d["fanout_calls"] == 2  # every result from the device
        for s, (ids_want, nodes_want, offs) in want.items():
            ids = np.concatenate([np.asarray(d[s]["seed_ids"], dtype=np.int64)
                                  for d in ranks])
            nodes = np.concatenate(
                [np.asarray(d[s]["nodes"], dtype=np.int64).reshape(-1, 19)
                 for d in ranks])
            order = np.argsort(ids, kind="stable")
            assert np.array_equal(ids[order], ids_want), (world, s)
            assert np.array_equal(nodes[order], nodes_want), (world, s)
            draws = int((nodes_want[:, 1:] >= 0).sum())
            for rank, d in enumerate(ranks):
                own = seeds[np.asarray(d[s]["seed_ids"], dtype=np.int64)]
                assert ((own // slice_) == rank).all(), (world, s, rank)
                assert d[s]["rounds"] == 2
                assert d[s]["draws"] == draws
                assert d[s]["bytes_coll"] > 0, (world, s, rank)
