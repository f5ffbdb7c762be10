"""Fan-out sampling without replacement (replace=False): the NumPy oracle,
tests of the oracle itself, and the host path of Engine.sample_neighbors
against it, exact.

Layout, level_offsets, seeds and the -1 conventions are those of
test_fanout_oracle.py; only the way a live parent fills its f children
changes. With r_c = draw(seed, i, col_c - 1) the draw of child c's column:

  domain   random (and edge_weight without weights): the deg slots of the
           stored row in order, m = deg. top_k: the m = min(deg, top_k)
           heaviest arcs, heaviest first, ties to the smaller slot (the first
           m slots without weights or when deg <= top_k).
  m <= f   child c < m takes domain element c, the others stay -1; no draw.
  m > f    Floyd's subset sampling in child order: J = m - f + c,
           t = index(r_c, J + 1), e_c = J if t is among e_0..e_{c-1} else t;
           child c takes domain element e_c.

edge_weight on a weighted graph is not defined without replacement.

The distribution checks are properties of the generator for seed 7, not of
any code under test."""
import itertools
import json
import os
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import grapehip
from golden_data import p2p31_dir
from grapehip.io import read_ldbc_edges
from test_fanout_oracle import (assert_same, fanout_oracle, level_offsets,
                                pick_port, small_seeds, small_simple_graph)
from test_sampler_draw_oracle import build_rows, draw, index

REPO = Path(__file__).resolve().parent.parent


def domain_slots(w_row, deg, strategy, top_k):
    """The ordered arc slots a parent draws from."""
    if strategy == "random" or (strategy == "edge_weight" and w_row is None):
        return list(range(deg))
    assert strategy == "top_k", "edge_weight needs replace=True with weights"
    m = min(deg, top_k)
    if w_row is None or deg <= top_k:
        return list(range(m))
    return sorted(range(deg), key=lambda i: (-float(w_row[i]), i))[:m]


def floyd(m, f, draws):
    """e_0..e_{f-1} out of 0..m-1, m > f; draws(c) is r_c."""
    e = []
    for c in range(f):
        J = m - f + c
        t = index(draws(c), J + 1)
        e.append(J if t in e else t)
    return e


def fanout_oracle_norep(num_v, src, dst, w, seeds, fanouts, strategy="random",
                        top_k=4, seed=7, directed=True, slots=None):
    """(seed_ids, nodes, level_offsets) of a world of one rank. slots: a dict
    that receives {(row, first child column): [arc slot of each live child]}."""
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
                dom = domain_slots(None if aw is None else aw[b:e], e - b,
                                   strategy, top_k)
                m = len(dom)
                first = int(offs[h]) + j * f
                if m <= f:
                    taken = dom
                else:
                    taken = [dom[x] for x in floyd(
                        m, f, lambda c: draw(seed, int(i), first + c - 1))]
                for c, slot in enumerate(taken):
                    nodes[row, first + c] = adj[b + slot]
                if slots is not None and taken:
                    slots[(row, first)] = list(taken)
    return seed_ids, nodes, offs


def star(n):
    return np.zeros(n, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64)


# --- the oracle itself ------------------------------------------------------

@pytest.mark.parametrize("strategy,top_k", (("random", 4), ("top_k", 3),
                                            ("top_k", 12)))
def test_children_are_distinct_slots(strategy, top_k):
    src, dst, w = small_simple_graph(True)
    off, adj, aw = build_rows(300, src, dst, w)
    for fanouts in ([3, 5, 2], [4], [40]):
        slots = {}
        ids, nodes, offs = fanout_oracle_norep(
            300, src, dst, w, small_seeds(), fanouts, strategy, top_k=top_k,
            slots=slots)
        assert len(ids) == 58 and len(slots) > 50
        parents = grapehip.fanout_parents(fanouts)
        for (row, first), taken in slots.items():
            v = int(nodes[row, parents[first]])
            deg = int(off[v + 1] - off[v])
            m = deg if strategy == "random" else min(deg, top_k)
            f = fanouts[int(np.searchsorted(offs, first, side="right")) - 2]
            assert len(taken) == min(m, f) == len(set(taken))
            assert all(0 <= s < deg for s in taken)
            # a simple graph: distinct slots are distinct vertices
            kids = nodes[row, first:first + f]
            assert (kids[len(taken):] == -1).all()
            assert len(set(kids[:len(taken)].tolist())) == len(taken)


def test_short_rows_come_back_whole():
    src, dst, w = small_simple_graph(True)
    off, adj, _ = build_rows(300, src, dst, w)
    seeds = small_seeds()
    ids, nodes, _ = fanout_oracle_norep(300, src, dst, w, seeds, [40])
    deg = np.diff(off)
    assert deg.max() <= 40 and deg[seeds[ids]].min() == 0
    for row, i in enumerate(ids):
        v = int(seeds[i])
        want = adj[off[v]:off[v + 1]].tolist()
        assert nodes[row, 1:].tolist() == want + [-1] * (40 - len(want))


def test_unit_fanouts_draw_with_replacement():
    seeds = small_seeds()
    src, dst, w = small_simple_graph(False)
    for weights, strategies in ((None, ("random", "edge_weight", "top_k")),
                                (w, ("random", "top_k"))):
        for strategy in strategies:
            a = fanout_oracle_norep(300, src, dst, weights, seeds, [1] * 4,
                                    strategy, top_k=3, seed=11,
                                    directed=False)
            b = fanout_oracle(300, src, dst, weights, seeds, [1] * 4,
                              strategy, top_k=3, seed=11, directed=False)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
            assert (a[1][:, -1] >= 0).sum() > 50


def test_dead_parent_blanks_its_subtree():
    # 0 -> {1, 2}, 1 -> 3, 2 and 3 are sinks
    src, dst = np.array([0, 0, 1]), np.array([1, 2, 3])
    _, nodes, offs = fanout_oracle_norep(4, src, dst, None, [0], [4, 2, 2])
    assert offs.tolist() == [0, 1, 5, 13, 29]
    row = nodes[0]
    assert row[1:5].tolist() == [1, 2, -1, -1]
    assert row[5:13].tolist() == [3, -1] + [-1] * 6
    assert (row[13:] == -1).all()


def test_top_k_children_lie_within_the_heaviest():
    src, dst, w = small_simple_graph(True)
    off, adj, aw = build_rows(300, src, dst, w)
    seeds = small_seeds()
    seen_long = 0
    for k, f in ((3, 5), (12, 4), (5, 5)):
        ids, nodes, _ = fanout_oracle_norep(300, src, dst, w, seeds, [f],
                                            "top_k", top_k=k)
        for row, i in enumerate(ids):
            v = int(seeds[i])
            b, e = int(off[v]), int(off[v + 1])
            order = sorted(range(e - b), key=lambda s: (-float(aw[b + s]), s))
            heavy = [int(adj[b + s]) for s in order[:k]]
            kids = [x for x in nodes[row, 1:].tolist() if x >= 0]
            assert len(kids) == min(e - b, k, f) and set(kids) <= set(heavy)
            if min(e - b, k) <= f and e - b > k:
                assert kids == heavy  # ranked, heaviest first
                seen_long += 1
    assert seen_long > 20


# --- uniformity of the generator, seed 7 ------------------------------------

def test_inclusion_is_uniform():
    # 4000 draws of 6 out of 40: each neighbour is in 4000 * 6/40 = 600 of
    # them, sd = sqrt(4000 * 0.15 * 0.85) = 22.6; within 4 sd
    src, dst = star(40)
    _, nodes, _ = fanout_oracle_norep(41, src, dst, None, [0] * 4000, [6])
    kids = nodes[:, 1:]
    assert (kids >= 1).all()
    assert all(len(set(r)) == 6 for r in kids.tolist())
    count = np.bincount(kids.ravel(), minlength=41)[1:]
    print("inclusion counts", count.min(), count.max())
    assert np.abs(count - 600).max() <= 90, count


def test_subsets_are_uniform():
    # 5000 draws of 2 out of 5: each of the 10 subsets 500 times, sd =
    # sqrt(5000 * 0.1 * 0.9) = 21.2; within 4 sd
    src, dst = star(5)
    _, nodes, _ = fanout_oracle_norep(6, src, dst, None, [0] * 5000, [2])
    count = Counter(tuple(sorted(r)) for r in nodes[:, 1:].tolist())
    print("subset counts", min(count.values()), max(count.values()))
    assert set(count) == set(itertools.combinations(range(1, 6), 2))
    assert all(abs(n - 500) <= 85 for n in count.values()), count


# --- the host path, world 1 -------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29771)


CASES = [("random", 3, f) for f in ([3, 5, 2], [4], [40], [])]
CASES += [("top_k", 3, f) for f in ([3, 5, 2], [4], [40], [])]
CASES += [("top_k", 12, [4])]


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("weighted", (True, False))
def test_host_exact(eng, directed, weighted):
    src, dst, w = small_simple_graph(directed)
    if not weighted:
        w = None
    seeds = small_seeds()
    g = eng.load_edges(src, dst, weights=w, directed=directed,
                       num_vertices=300)
    cases = list(CASES)
    if not weighted:
        cases += [("edge_weight", 3, f) for f in ([3, 5, 2], [4], [40])]
    deg = np.diff(build_rows(300, src, dst, w, directed)[0])
    assert (deg > 12).any() and (deg < 4).any()  # m > f and m <= f occur
    for strategy, k, fanouts in cases:
        want = fanout_oracle_norep(300, src, dst, w, seeds, fanouts, strategy,
                                   top_k=k, seed=7, directed=directed)
        assert len(want[0]) == 58
        r = eng.sample_neighbors(g, seeds, fanouts, strategy=strategy,
                                 top_k=k, seed=7, replace=False)
        assert_same(r, want, (strategy, k, fanouts))
        assert "traversed_edges" not in r  # the host path
        with_r = eng.sample_neighbors(g, seeds, fanouts, strategy=strategy,
                                      top_k=k, seed=7, replace=True)
        assert sorted(r) == sorted(with_r)  # the same keys
        if fanouts:
            assert not np.array_equal(r["nodes"], with_r["nodes"])
    # another seed
    a = eng.sample_neighbors(g, seeds, [4], seed=8, replace=False)
    assert_same(a, fanout_oracle_norep(300, src, dst, w, seeds, [4], seed=8,
                                       directed=directed))


def test_host_unit_fanouts_and_whole_rows(eng):
    src, dst, w = small_simple_graph(True)
    seeds = small_seeds()
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    for strategy in ("random", "top_k"):
        a = eng.sample_neighbors(g, seeds, [1] * 4, strategy=strategy,
                                 top_k=3, replace=False)
        b = eng.sample_neighbors(g, seeds, [1] * 4, strategy=strategy,
                                 top_k=3)
        assert np.array_equal(a["nodes"], b["nodes"])
    # a fan-out no row reaches: every row once, in stored order
    off, adj, _ = build_rows(300, src, dst, w)
    r = eng.sample_neighbors(g, seeds, [40], replace=False)
    for row, i in zip(r["nodes"], r["seed_ids"]):
        v = int(seeds[i])
        want = adj[off[v]:off[v + 1]].tolist()
        assert row[1:].tolist() == want + [-1] * (40 - len(want))


# --- errors and the default -------------------------------------------------

def test_errors_and_default(eng):
    src, dst, w = small_simple_graph(True)
    seeds = small_seeds()
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    with pytest.raises(RuntimeError, match="edge_weight") as err:
        eng.sample_neighbors(g, seeds, [2], strategy="edge_weight",
                             replace=False)
    assert "replace=False" in str(err.value)
    with pytest.raises(RuntimeError, match="fanout = 0"):
        eng.sample_neighbors(g, seeds, [2, 0], replace=False)
    with pytest.raises(RuntimeError, match="top_k = 0"):
        eng.sample_neighbors(g, seeds, [2], strategy="top_k", top_k=0,
                             replace=False)
    # replace=True is the call without the keyword, bit for bit
    for strategy in ("random", "edge_weight", "top_k"):
        a = eng.sample_neighbors(g, seeds, [3, 5, 2], strategy=strategy,
                                 top_k=3, replace=True)
        b = eng.sample_neighbors(g, seeds, [3, 5, 2], strategy=strategy,
                                 top_k=3)
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), (strategy, key)
        assert_same(a, fanout_oracle(300, src, dst, w, seeds, [3, 5, 2],
                                     strategy, top_k=3))


# --- the host path, world 2 -------------------------------------------------

NOREP_WORKER = r'''
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
for strategy in ("random", "top_k"):
    r = eng.sample_neighbors(g, d["seeds"], [3, 5, 2], strategy=strategy,
                             top_k=3, seed=7, replace=False)
    out[strategy] = {"seed_ids": r["seed_ids"].tolist(),
                     "nodes": r["nodes"].tolist(),
                     "level_offsets": r["level_offsets"].tolist()}
path = os.path.join(os.environ["GRAPEHIP_OUT"],
                    "rank%s.json" % os.environ["RANK"])
json.dump(out, open(path, "w"))
'''


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
        procs.append(subprocess.Popen([sys.executable, "-c", NOREP_WORKER],
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
    for s in ("random", "top_k"):
        one = eng.sample_neighbors(g, seeds, [3, 5, 2], strategy=s, top_k=3,
                                   seed=7, replace=False)
        assert_same(one, fanout_oracle_norep(300, src, dst, w, seeds,
                                             [3, 5, 2], s, top_k=3,
                                             directed=False), s)
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

def test_cli_sample_replace(tmp_path):
    data = p2p31_dir()
    src, dst, _ = read_ldbc_edges(str(data / "p2p-31.e"), weighted=True)
    nbrs = {}
    for a, b in zip(src.tolist(), dst.tolist()):
        nbrs.setdefault(a, Counter())[b] += 1
        nbrs.setdefault(b, Counter())[a] += 1
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application",
           "sample", "--sample_walks", "40", "--sample_fanout", "2-3",
           "--sample_replace", "0", "--sample_seed", "9", "--efile",
           str(data / "p2p-31.e"), "--out_prefix", str(out)]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [list(map(int, line.split()))
            for line in open(out / "result_frag_0").read().splitlines()]
    assert [row[0] for row in rows] == list(range(40))
    families = short = 0
    for row in rows:
        assert len(row) == 1 + 8
        groups = [(row[0], row[1:3])]
        groups += [(row[1 + j], row[3 + 3 * j:6 + 3 * j]) for j in range(2)]
        for parent, kids in groups:
            live = [k for k in kids if k >= 0]
            assert kids == live + [-1] * (len(kids) - len(live)), row
            if parent < 0 or parent not in nbrs:
                assert not live, row
                continue
            row_of = nbrs[parent]
            deg = sum(row_of.values())
            # distinct arcs of the parent: as many as the row or the fan-out
            assert len(live) == min(deg, len(kids)), row
            assert not Counter(live) - row_of, row
            if max(row_of.values()) == 1:
                assert len(set(live)) == len(live), row
            families += 1
            short += deg < len(kids)
    assert families >= 30 and short >= 1
