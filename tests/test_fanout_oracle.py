"""Fan-out (neighbourhood) sampling: the NumPy oracle, tests of the oracle
itself, and the host path of Engine.sample_neighbors against it, exact.

One specification for oracle, host and device. With fanouts f_1..f_H,
L_0 = 1, L_h = L_{h-1} * f_h, S = L_1 + ... + L_H and base_h = L_1 + ... +
L_{h-1}, the row of a seed is 1 + S ids: column 0 the seed, column 1 + pos
sample slot pos; level h holds the slots base_h .. base_h + L_h - 1, and slot
base_h + j has its children in the slots base_{h+1} + j * f_{h+1} + c. The
draw of slot pos of seed index i is draw(seed, i, pos) of
test_sampler_draw_oracle, the arc is pick_slot of the parent's stored row;
a dead parent leaves its whole subtree -1.

Exact comparisons run on simple graphs (unique pairs, quarter weights), so
every fp32 row sum is exact and parallel arcs, whose order is unspecified, do
not occur."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import grapehip
from golden_data import p2p31_dir
from grapehip.io import read_ldbc_edges
from test_sampler_draw_oracle import build_rows, draw, pick_slot, walk_oracle

REPO = Path(__file__).resolve().parent.parent
STRATEGIES = ("random", "edge_weight", "top_k")


def level_offsets(fanouts):
    offs, length = [0, 1], 1
    for f in fanouts:
        length *= f
        offs.append(offs[-1] + length)
    return np.array(offs, dtype=np.int64)


def fanout_oracle(num_v, src, dst, w, seeds, fanouts, strategy="random",
                  top_k=4, seed=7, directed=True):
    """(seed_ids, nodes, level_offsets) of a world of one rank."""
    off, adj, aw = build_rows(num_v, src, dst, w, directed)
    seeds = np.asarray(seeds, dtype=np.int64)
    seed_ids = np.nonzero((seeds >= 0) & (seeds < num_v))[0].astype(np.int64)
    offs = level_offsets(fanouts)
    nodes = np.full((len(seed_ids), offs[-1]), -1, dtype=np.int64)
    for row, i in enumerate(seed_ids):
        nodes[row, 0] = seeds[i]
        for h, f in enumerate(fanouts, start=1):
            for j in range(offs[h] - offs[h - 1]):  # the parents, level h - 1
                v = int(nodes[row, offs[h - 1] + j])
                if v < 0:
                    continue
                b, e = int(off[v]), int(off[v + 1])
                if e == b:
                    continue
                for c in range(f):
                    col = int(offs[h]) + j * f + c
                    slot = pick_slot(draw(seed, int(i), col - 1),
                                     None if aw is None else aw[b:e], e - b,
                                     strategy, top_k)
                    if slot is not None:
                        nodes[row, col] = adj[b + slot]
    return seed_ids, nodes, offs


def oracle_counts(nodes, offs):
    """(rounds, draws) as the device path reports them: the levels that began
    with a live parent somewhere, and the samples drawn."""
    rounds = 0
    for h in range(1, len(offs) - 1):
        if not (nodes[:, offs[h - 1]:offs[h]] >= 0).any():
            break
        rounds += 1
    return rounds, int((nodes[:, 1:] >= 0).sum())


def quarter_weights(rng, n):
    return (rng.integers(4, 41, size=n) / 4.0).astype(np.float32)


def small_simple_graph(directed, num_v=300, arcs=2400, seed=301):
    """Unique pairs without self-loops over 0..num_v-2 (the last vertex stays
    isolated); undirected: arcs/2 unique unordered pairs."""
    rng = np.random.default_rng(seed + int(directed))
    want = arcs if directed else arcs // 2
    a = rng.integers(0, num_v - 1, size=3 * want)
    b = rng.integers(0, num_v - 1, size=3 * want)
    keep = a != b
    a, b = a[keep], b[keep]
    if not directed:
        a, b = np.minimum(a, b), np.maximum(a, b)
    _, first = np.unique(a * num_v + b, return_index=True)
    first = np.sort(first)[:want]
    assert len(first) == want
    return (a[first].astype(np.int64), b[first].astype(np.int64),
            quarter_weights(rng, want))


def small_seeds(num_v=300, seed=303):
    """Duplicates, two ids that are no vertex, the isolated vertex."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, num_v - 1, size=56)
    s[20:25] = s[0:5]
    return np.concatenate([s, [num_v - 1, num_v + 40, -1, s[3]]]).astype(
        np.int64)


def assert_same(r, want, ctx=None):
    ids, nodes, offs = want
    assert r["seed_ids"].dtype == np.int64 and r["nodes"].dtype == np.int64
    assert np.array_equal(r["seed_ids"], ids), ctx
    assert np.array_equal(r["level_offsets"], offs), ctx
    assert r["nodes"].shape == nodes.shape, ctx
    bad = np.nonzero((r["nodes"] != nodes).any(axis=1))[0]
    assert len(bad) == 0, (ctx, bad[:5], r["nodes"][bad[:5]], nodes[bad[:5]])


# --- the oracle itself ------------------------------------------------------

def test_layout():
    fanouts = [3, 5, 2]
    offs = level_offsets(fanouts)
    assert offs.tolist() == [0, 1, 4, 19, 49]
    # every sample is a neighbour of the slot the layout formula names
    src, dst, w = small_simple_graph(True)
    _, nodes, got = fanout_oracle(300, src, dst, w, [5, 17], fanouts)
    assert np.array_equal(got, offs)
    arcs = set(zip(src.tolist(), dst.tolist()))
    L = np.diff(offs)  # 1, 3, 15, 30
    base = offs[1:] - 1  # base_h of level h = 1.. as sample slots
    for row in nodes:
        for c in range(3):  # the children of the seed: slots 0..f_1-1
            assert (int(row[0]), int(row[1 + c])) in arcs
        for h in (1, 2):
            f = fanouts[h]
            for j in range(L[h]):
                parent = int(row[1 + base[h - 1] + j])
                for c in range(f):
                    child = int(row[1 + base[h] + j * f + c])
                    assert parent >= 0 and (parent, child) in arcs


def test_unit_fanouts_are_walks():
    src, dst, w = small_simple_graph(False)
    seeds = small_seeds()
    for strategy in STRATEGIES:
        ids, nodes, _ = fanout_oracle(300, src, dst, w, seeds, [1] * 4,
                                      strategy, top_k=3, seed=11,
                                      directed=False)
        wid, paths = walk_oracle(300, src, dst, w, seeds, 4, strategy,
                                 top_k=3, seed=11, directed=False)
        assert np.array_equal(ids, wid) and np.array_equal(nodes, paths)
        assert (nodes[:, -1] >= 0).sum() > 50


def test_no_levels_duplicates_and_invalid_seeds():
    src, dst = np.array([0, 1]), np.array([1, 2])
    ids, nodes, offs = fanout_oracle(4, src, dst, None, [2, 9, 0, -1, 0], [])
    assert ids.tolist() == [0, 2, 4] and offs.tolist() == [0, 1]
    assert nodes.tolist() == [[2], [0], [0]]
    assert oracle_counts(nodes, offs) == (0, 0)
    # duplicates draw with their own seed index
    src = np.zeros(40, dtype=np.int64)
    dst = np.arange(1, 41, dtype=np.int64)
    ids, nodes, _ = fanout_oracle(41, src, dst, None, [0, 0, 77, 0], [6])
    assert ids.tolist() == [0, 1, 3]
    assert len({tuple(r) for r in nodes.tolist()}) == 3


def test_dead_parent_blanks_its_subtree():
    # 0 -> {1, 2}, 1 -> 3, 2 and 3 are sinks
    src, dst = np.array([0, 0, 1]), np.array([1, 2, 3])
    _, nodes, offs = fanout_oracle(4, src, dst, None, [0], [4, 2, 2], seed=3)
    row = nodes[0]
    lvl1 = row[1:5]
    assert set(lvl1.tolist()) == {1, 2}  # both children occur for seed 3
    for j, v in enumerate(lvl1):
        kids = row[5 + 2 * j:7 + 2 * j]
        assert kids.tolist() == ([3, 3] if v == 1 else [-1, -1])
        for c in range(2):
            assert (row[13 + (2 * j + c) * 2:15 + (2 * j + c) * 2] == -1).all()
    # level 3 began with live parents (the 3s), and drew nothing
    assert oracle_counts(nodes, offs) == (3, 4 + 2 * int((lvl1 == 1).sum()))
    # a row whose weights sum to nothing is a dead end for edge_weight only
    w = np.array([0.0, 0.0, 1.0], dtype=np.float32)
    _, nodes, offs = fanout_oracle(4, src, dst, w, [0], [2, 2], "edge_weight")
    assert nodes.tolist() == [[0] + [-1] * 6]
    assert oracle_counts(nodes, offs) == (1, 0)


@pytest.mark.parametrize("fanouts", ([3, 5, 2], [1], []))
def test_fanout_parents(fanouts):
    offs = level_offsets(fanouts)
    want = np.full(offs[-1], -1, dtype=np.int64)
    for h in range(1, len(fanouts) + 1):
        for j in range(offs[h] - offs[h - 1]):
            for c in range(fanouts[h - 1]):
                want[offs[h] + j * fanouts[h - 1] + c] = offs[h - 1] + j
    got = grapehip.fanout_parents(fanouts)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (got[1:] >= 0).all() and got[0] == -1


# --- the host path, world 1 -------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29751)


@pytest.mark.parametrize("directed", (True, False))
def test_host_exact(eng, directed):
    src, dst, w = small_simple_graph(directed)
    seeds = small_seeds()
    g = eng.load_edges(src, dst, weights=w, directed=directed,
                       num_vertices=300)
    for strategy in STRATEGIES:
        for fanouts in ([3, 5, 2], [4]):
            want = fanout_oracle(300, src, dst, w, seeds, fanouts, strategy,
                                 top_k=3, seed=7, directed=directed)
            assert len(want[0]) == 58
            assert (want[1][:, want[2][-2]:] >= 0).mean() > 0.8
            r = eng.sample_neighbors(g, seeds, fanouts, strategy=strategy,
                                     top_k=3, seed=7)
            assert_same(r, want, (strategy, fanouts))
            assert "traversed_edges" not in r  # the host path
    # the default strategy and seed, no levels, another seed
    assert_same(eng.sample_neighbors(g, seeds, [2, 2]),
                fanout_oracle(300, src, dst, w, seeds, [2, 2],
                              directed=directed))
    assert_same(eng.sample_neighbors(g, seeds, []),
                fanout_oracle(300, src, dst, w, seeds, [], directed=directed))
    a = eng.sample_neighbors(g, seeds, [4], seed=8)
    assert not np.array_equal(a["nodes"], r["nodes"])


def test_host_unweighted_and_dead_ends(eng):
    src, dst, _ = small_simple_graph(True)
    seeds = small_seeds()
    g = eng.load_edges(src, dst, directed=True, num_vertices=300)
    for strategy in STRATEGIES:
        r = eng.sample_neighbors(g, seeds, [2, 3], strategy=strategy, top_k=2,
                                 seed=5)
        assert_same(r, fanout_oracle(300, src, dst, None, seeds, [2, 3],
                                     strategy, top_k=2, seed=5), strategy)
    # 0 -> 1 -> 2 -> 3 -> 4 (a sink); 10 -> {11, 12} with weights 0
    src = np.array([0, 1, 2, 3, 10, 10], dtype=np.int64)
    dst = np.array([1, 2, 3, 4, 11, 12], dtype=np.int64)
    w = np.array([1, 1, 1, 1, 0, 0], dtype=np.float32)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=13)
    r = eng.sample_neighbors(g, [0], [2] * 6)
    offs = r["level_offsets"]
    assert offs.tolist() == [0, 1, 3, 7, 15, 31, 63, 127]
    for h, v in enumerate((0, 1, 2, 3, 4)):
        assert (r["nodes"][0, offs[h]:offs[h + 1]] == v).all()
    assert (r["nodes"][0, offs[5]:] == -1).all()
    r = eng.sample_neighbors(g, [10, 10], [2, 2], strategy="edge_weight")
    assert r["nodes"].tolist() == [[10] + [-1] * 6] * 2
    r = eng.sample_neighbors(g, [10], [8], strategy="random")
    assert set(r["nodes"][0, 1:].tolist()) == {11, 12}


def test_host_arbitrary_oids(eng):
    src, dst, w = small_simple_graph(False)
    rng = np.random.default_rng(305)
    oids = rng.choice(10 ** 12, size=300, replace=False).astype(np.int64)
    g = eng.load_edges(oids[src], oids[dst], weights=w, directed=False,
                       vertex_oids=oids, idxer="hashmap")
    arcs = set(zip(oids[src].tolist(), oids[dst].tolist()))
    arcs |= {(b, a) for a, b in arcs}
    seeds = np.concatenate([oids[:40], [5, -7]])
    parents = grapehip.fanout_parents([3, 2])
    for strategy in STRATEGIES:
        r = eng.sample_neighbors(g, seeds, [3, 2], strategy=strategy)
        assert np.array_equal(r["seed_ids"], np.arange(40))
        assert np.array_equal(r["nodes"][:, 0], oids[:40])
        live = 0
        for row in r["nodes"]:
            for c in range(1, 10):
                if row[c] >= 0:
                    assert (int(row[parents[c]]), int(row[c])) in arcs
                    live += 1
        assert live > 300


# --- errors -----------------------------------------------------------------

def test_errors(eng):
    src, dst, w = small_simple_graph(True)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    seeds = np.arange(3, dtype=np.int64)
    with pytest.raises(RuntimeError, match="fanout = 0"):
        eng.sample_neighbors(g, seeds, [2, 0])
    with pytest.raises(RuntimeError, match="fanout = -3"):
        eng.sample_neighbors(g, seeds, [-3])
    # 3 * (1 + 1000 + 10^6 + 10^9) entries is above the cap of 2^31
    with pytest.raises(RuntimeError, match="1000-1000-1000"):
        eng.sample_neighbors(g, seeds, [1000, 1000, 1000])
    # sizes that overflow 64 bits are caught by the same check
    with pytest.raises(RuntimeError, match="kFanoutMaxEntries"):
        eng.sample_neighbors(g, seeds, [2 ** 31] * 4)
    with pytest.raises(RuntimeError, match="random|edge_weight|top_k"):
        eng.sample_neighbors(g, seeds, [2], strategy="alias")
    with pytest.raises(RuntimeError, match="top_k = 0"):
        eng.sample_neighbors(g, seeds, [2], strategy="top_k", top_k=0)
    with pytest.raises(RuntimeError, match="gpu=True"):
        eng.sample_neighbors(g, seeds, [2], device=True)
    with pytest.raises(ValueError, match="fanout = 0"):
        grapehip.fanout_parents([2, 0])


# --- the host path, world 2 -------------------------------------------------

HOST_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
import numpy as np
import grapehip
eng = grapehip.engine_from_env()
d = np.load(os.environ["GRAPEHIP_GRAPH"])
sl = slice(eng.rank, None, eng.world)
g = eng.load_edges(d["src"][sl], d["dst"][sl], weights=d["w"][sl],
                   directed=False, num_vertices=int(d["num_v"]))
out = {}
for strategy in ("random", "edge_weight", "top_k"):
    r = eng.sample_neighbors(g, d["seeds"], [3, 5, 2], strategy=strategy,
                             top_k=3, seed=7)
    out[strategy] = {"seed_ids": r["seed_ids"].tolist(),
                     "nodes": r["nodes"].tolist(),
                     "level_offsets": r["level_offsets"].tolist()}
path = os.path.join(os.environ["GRAPEHIP_OUT"],
                    "rank%s.json" % os.environ["RANK"])
json.dump(out, open(path, "w"))
'''


def pick_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_host_world_of_two(eng, tmp_path):
    src, dst, w = small_simple_graph(False)
    seeds = small_seeds()
    graph_file = tmp_path / "graph.npz"
    np.savez(graph_file, src=src, dst=dst, w=w, seeds=seeds, num_v=300)
    port = pick_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, GRAPEHIP_REPO=str(REPO),
                   GRAPEHIP_OUT=str(tmp_path), GRAPEHIP_GRAPH=str(graph_file),
                   RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", HOST_WORKER],
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
    ranks = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in (0, 1)]
    g = eng.load_edges(src, dst, weights=w, directed=False, num_vertices=300)
    for s in STRATEGIES:
        one = eng.sample_neighbors(g, seeds, [3, 5, 2], strategy=s, top_k=3,
                                   seed=7)
        a, b = (np.asarray(d[s]["seed_ids"], dtype=np.int64) for d in ranks)
        assert len(a) and len(b) and not set(a.tolist()) & set(b.tolist())
        ids = np.concatenate([a, b])
        nodes = np.concatenate(
            [np.asarray(d[s]["nodes"], dtype=np.int64).reshape(-1, 49)
             for d in ranks])
        order = np.argsort(ids, kind="stable")
        assert np.array_equal(ids[order], one["seed_ids"]), s
        assert np.array_equal(nodes[order], one["nodes"]), s
        for d in ranks:
            assert d[s]["level_offsets"] == [0, 1, 4, 19, 49]


# --- CLI --------------------------------------------------------------------

def test_cli_sample_fanout(tmp_path):
    data = p2p31_dir()
    src, dst, _ = read_ldbc_edges(str(data / "p2p-31.e"), weighted=True)
    arcs = set(zip(src.tolist(), dst.tolist()))
    arcs |= {(b, a) for a, b in arcs}
    vertices = set(src.tolist()) | set(dst.tolist())
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application",
           "sample", "--sample_walks", "40", "--sample_fanout", "2-3",
           "--sample_seed", "9", "--efile", str(data / "p2p-31.e"),
           "--out_prefix", str(out)]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [list(map(int, line.split()))
            for line in open(out / "result_frag_0").read().splitlines()]
    seeds = [row[0] for row in rows]
    # one row per seed 0..39; the ids without an edge are isolated vertices
    assert seeds == list(range(40)) and len(vertices & set(seeds)) >= 10
    parents = grapehip.fanout_parents([2, 3])
    live = 0
    for row in rows:
        assert len(row) == 1 + 8
        for c in range(1, 9):
            if row[c] >= 0:
                assert (row[parents[c]], row[c]) in arcs, row
                live += 1
            else:
                assert row[parents[c]] < 0 or row[parents[c]] not in vertices
    assert live >= 80
