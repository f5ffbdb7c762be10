"""Device random-walk sampler on one MI355X: the HIP path against the
NumPy oracle of test_sampler_draw_oracle.py, path for path.

Exact comparisons run on simple graphs (unique (src, dst) pairs, no
self-loops, identity ids) with weights j/4, j in 4..40: every fp32 row sum is
then exact in any summation order, so the association of the device scan
cannot show. Every device call asserts that the `_debug_sample` call counter
moved: a silent host fallback fails.

`rounds` counts the hops that began with a live walk somewhere, so a run whose
walks all died stops early."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import grapehip
from test_gpu_kcore import multigraph, pick_port
from test_sampler_draw_oracle import build_rows, walk_oracle

REPO = Path(__file__).resolve().parent.parent
STRATEGIES = ("random", "edge_weight", "top_k")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29741, gpu=True)


def device_sample(eng, g, starts, **kw):
    """sample on the device: the call counter must move."""
    before = eng._debug_sample()["calls"]
    r = eng.sample(g, np.asarray(starts, dtype=np.int64), device=True, **kw)
    assert eng._debug_sample()["calls"] == before + 1
    for key in ("rounds", "seconds", "traversed_edges", "bytes_p2p",
                "bytes_coll"):
        assert key in r, key
    assert r["walk_ids"].dtype == np.int64 and r["paths"].dtype == np.int64
    return r


def quarter_weights(rng, n):
    return (rng.integers(4, 41, size=n) / 4.0).astype(np.float32)


def simple_graph(directed, num_v=2000, arcs=16000, seed=201):
    """Unique pairs without self-loops over the vertices 0..num_v-2 (the last
    vertex stays isolated); undirected: arcs/2 unique unordered pairs."""
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
    src, dst = a[first].astype(np.int64), b[first].astype(np.int64)
    return src, dst, quarter_weights(rng, want)


def graph1_starts(num_v=2000, seed=203):
    """500 walks: duplicates, two ids that are no vertex, the isolated one."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, num_v - 1, size=496)
    s[100:110] = s[0:10]
    return np.concatenate([s, [num_v - 1, num_v + 500, -1, s[3]]]).astype(
        np.int64)


def assert_same(r, want, ctx=None):
    ids, paths = want
    assert np.array_equal(r["walk_ids"], ids), ctx
    assert r["paths"].shape == paths.shape, ctx
    bad = np.nonzero((r["paths"] != paths).any(axis=1))[0]
    assert len(bad) == 0, (ctx, bad[:5], r["paths"][bad[:5]], paths[bad[:5]])


# --- 1. exact against the oracle --------------------------------------------

@pytest.mark.parametrize("directed", (True, False))
def test_exact_all_strategies(eng, directed):
    src, dst, w = simple_graph(directed)
    starts = graph1_starts()
    g = eng.load_edges(src, dst, weights=w, directed=directed,
                       num_vertices=2000)
    for strategy in STRATEGIES:
        want = walk_oracle(2000, src, dst, w, starts, 4, strategy, top_k=4,
                           seed=7, directed=directed)
        assert len(want[0]) == 498 and (want[1][:, -1] >= 0).sum() > 400
        r = device_sample(eng, g, starts, hops=4, strategy=strategy, top_k=4,
                          seed=7)
        assert_same(r, want, strategy)
        assert r["traversed_edges"] == int((want[1][:, 1:] >= 0).sum())
        assert r["rounds"] == 4
        assert r["bytes_p2p"] == 0
    # hops=0: the starts alone
    r = device_sample(eng, g, starts, hops=0)
    assert_same(r, walk_oracle(2000, src, dst, w, starts, 0,
                               directed=directed))
    assert r["rounds"] == 0 and r["traversed_edges"] == 0


def test_unweighted_edge_weight_equals_random(eng):
    src, dst, _ = simple_graph(True)
    starts = graph1_starts()
    g = eng.load_edges(src, dst, directed=True, num_vertices=2000)
    eng._debug_sample(reset=True)
    a = device_sample(eng, g, starts, hops=3, strategy="edge_weight", seed=3)
    b = device_sample(eng, g, starts, hops=3, strategy="random", seed=3)
    assert np.array_equal(a["paths"], b["paths"])
    assert_same(a, walk_oracle(2000, src, dst, None, starts, 3, "edge_weight",
                               seed=3))
    c = device_sample(eng, g, starts, hops=3, strategy="top_k", top_k=2,
                      seed=3)
    assert_same(c, walk_oracle(2000, src, dst, None, starts, 3, "top_k",
                               top_k=2, seed=3))
    hook = eng._debug_sample()
    assert hook["cdf_builds"] == 0 and hook["topk_builds"] == 0


# --- 2. the row tiers of the index builds -----------------------------------

# thread per row up to 8 arcs, wave per row up to 1024 (64 arcs per trip),
# block per row beyond (256 arcs per chunk: the hub takes 20 chunks); and
# deg < k, == k, == k + 1 for k in 1, 3, 32
TIER_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 34, 63, 64, 65, 1023, 1024,
             1025, 5000)


def tier_graph():
    rng = np.random.default_rng(211)
    num_v = 5400
    src, dst = [], []
    for v, length in enumerate(TIER_LENS):
        src.append(np.full(length, v, dtype=np.int64))
        dst.append(np.sort(rng.choice(np.arange(100, num_v), size=length,
                                      replace=False)).astype(np.int64))
    src, dst = np.concatenate(src), np.concatenate(dst)
    return num_v, src, dst, quarter_weights(rng, len(src))


def test_row_tiers(eng):
    num_v, src, dst, w = tier_graph()
    # 37 weight values over rows of up to 5000 arcs: ties everywhere, decided
    # by the slot order; the hub's fp32 total stays exact (< 2^24 quarters)
    assert len(np.unique(w)) == 37 and w.sum() * 4 < 2 ** 24
    starts = np.repeat(np.arange(len(TIER_LENS)), 64)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=num_v)
    cases = [("edge_weight", 4), ("random", 4), ("top_k", 1), ("top_k", 3),
             ("top_k", 32)]
    for strategy, k in cases:
        want = walk_oracle(num_v, src, dst, w, starts, 1, strategy, top_k=k,
                           seed=7)
        r = device_sample(eng, g, starts, hops=1, strategy=strategy, top_k=k,
                          seed=7)
        assert_same(r, want, (strategy, k))
    # the picks of the hub spread over its chunks
    hub = want[1][starts == len(TIER_LENS) - 1, 1]
    assert len(np.unique(hub)) > 10


# --- 3. dead ends -------------------------------------------------------------

def test_dead_ends(eng):
    # 0 -> 1 -> 2 -> 3 -> 4 (a sink); 10 -> {11, 12} with weights 0
    src = np.array([0, 1, 2, 3, 10, 10], dtype=np.int64)
    dst = np.array([1, 2, 3, 4, 11, 12], dtype=np.int64)
    w = np.array([1, 1, 1, 1, 0, 0], dtype=np.float32)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=13)
    for strategy in STRATEGIES:
        r = device_sample(eng, g, [0, 2], hops=8, strategy=strategy)
        assert r["paths"].tolist() == [[0, 1, 2, 3, 4, -1, -1, -1, -1],
                                       [2, 3, 4, -1, -1, -1, -1, -1, -1]]
        # the walk from 0 is still live when hop 4 begins and dies in it
        assert r["rounds"] == 5 and r["traversed_edges"] == 6
    r = device_sample(eng, g, [10, 10, 4], hops=2, strategy="edge_weight")
    assert r["paths"].tolist() == [[10, -1, -1]] * 2 + [[4, -1, -1]]
    assert r["rounds"] == 1 and r["traversed_edges"] == 0
    r = device_sample(eng, g, [10, 10, 10, 10], hops=2, strategy="random")
    assert set(r["paths"][:, 1].tolist()) <= {11, 12}
    assert (r["paths"][:, 2] == -1).all() and r["rounds"] == 2
    assert_same(r, walk_oracle(13, src, dst, w, [10] * 4, 2, "random"))


# --- 4. index reuse -------------------------------------------------------------

def test_index_reuse(eng):
    src, dst, w = simple_graph(True, num_v=300, arcs=2000, seed=221)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    starts = np.arange(64)
    eng._debug_sample(reset=True)
    device_sample(eng, g, starts, strategy="random")
    hook = eng._debug_sample()
    assert hook["cdf_builds"] == 0 and hook["topk_builds"] == 0
    device_sample(eng, g, starts, strategy="edge_weight")
    device_sample(eng, g, starts, strategy="edge_weight", seed=8)
    assert eng._debug_sample()["cdf_builds"] == 1
    first = device_sample(eng, g, starts, strategy="top_k", top_k=3)
    again = device_sample(eng, g, starts, strategy="top_k", top_k=3)
    assert eng._debug_sample()["topk_builds"] == 1
    assert np.array_equal(first["paths"], again["paths"])
    r5 = device_sample(eng, g, starts, strategy="top_k", top_k=5)
    hook = eng._debug_sample()
    assert hook["topk_builds"] == 2 and hook["cdf_builds"] == 1
    assert hook["calls"] == 6
    assert hook["steps"] == r5["traversed_edges"] > 0
    assert_same(r5, walk_oracle(300, src, dst, w, starts, 2, "top_k",
                                top_k=5))


# --- 5. device-only graph -------------------------------------------------------

@pytest.fixture(scope="module")
def synthetic(eng):
    return eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7,
                              weighted=True)


def test_device_only_graph(eng, synthetic):
    """No host fragment: the default now walks on the device. The generator
    keeps its edges on the device, so a step is checked through bfs: its
    target is at depth 1 of its origin (a repeated vertex would be a
    self-loop, which bfs cannot show, and is not checked)."""
    starts = np.arange(0, 20000, 40, dtype=np.int64)
    runs = {}
    for strategy in STRATEGIES:
        before = eng._debug_sample()["calls"]
        r = eng.sample(synthetic, starts, hops=3, strategy=strategy, seed=5)
        assert eng._debug_sample()["calls"] == before + 1
        assert np.array_equal(r["walk_ids"], np.arange(500))
        assert np.array_equal(r["paths"][:, 0], starts)
        assert r["paths"].max() < 20000 and r["paths"].min() >= -1
        assert r["traversed_edges"] == int((r["paths"][:, 1:] >= 0).sum()) > 0
        again = eng.sample(synthetic, starts, hops=3, strategy=strategy,
                           seed=5)
        assert np.array_equal(again["paths"], r["paths"])
        other = eng.sample(synthetic, starts, hops=3, strategy=strategy,
                           seed=6)
        assert not np.array_equal(other["paths"], r["paths"])
        runs[strategy] = r["paths"]
    assert not np.array_equal(runs["random"], runs["top_k"])
    checked = 0
    for strategy in STRATEGIES:
        full = runs[strategy][(runs[strategy] >= 0).all(axis=1)][:3]
        for path in full:
            for h in range(3):
                a, b = int(path[h]), int(path[h + 1])
                if a == b:
                    continue
                d = eng.bfs(synthetic, a)
                depth = np.asarray(d["values"])[np.argsort(d["oids"])]
                assert depth[b] == 1, (strategy, path, h)
                checked += 1
    assert checked >= 20


# --- 6. no rerouting, limits ----------------------------------------------------

def test_host_fragment_keeps_the_host_path(eng):
    src, dst, w = simple_graph(True, num_v=300, arcs=2000, seed=231)
    g = eng.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    starts = np.arange(100, dtype=np.int64)
    top_k_max = eng._debug_sample()["top_k_max"]
    assert top_k_max == 32
    for strategy in STRATEGIES:
        before = eng._debug_sample()["calls"]
        a = eng.sample(g, starts, hops=3, strategy=strategy, seed=11)
        b = eng.sample(g, starts, hops=3, strategy=strategy, seed=11,
                       device=False)
        assert eng._debug_sample()["calls"] == before
        assert np.array_equal(a["walk_ids"], b["walk_ids"])
        assert np.array_equal(a["paths"], b["paths"])
        assert "traversed_edges" not in a
    with pytest.raises(RuntimeError, match="top_k = 33"):
        eng.sample(g, starts, strategy="top_k", top_k=top_k_max + 1,
                   device=True)
    with pytest.raises(RuntimeError, match="top_k = 0"):
        eng.sample(g, starts, strategy="top_k", top_k=0, device=True)
    cpu = grapehip.Engine(rank=0, world=1, master_port=29742)
    gc = cpu.load_edges(src, dst, weights=w, directed=True, num_vertices=300)
    with pytest.raises(RuntimeError, match="gpu=True"):
        cpu.sample(gc, starts, device=True)
    assert np.array_equal(cpu.sample(gc, starts, hops=3, seed=11)["paths"],
                          eng.sample(g, starts, hops=3, seed=11)["paths"])


# --- 7. multigraph: validity and determinism -----------------------------------

def test_multigraph_validity(eng):
    src, dst = multigraph(num_v=400, num_e=5000, loops=15, seed=241)
    rng = np.random.default_rng(242)
    w = (rng.random(len(src), dtype=np.float32) * 9 + 1)
    g = eng.load_edges(src, dst, weights=w, directed=False, num_vertices=400)
    arcs = set(zip(src.tolist(), dst.tolist())) | set(
        zip(dst.tolist(), src.tolist()))
    starts = rng.integers(0, 400, size=300)
    for strategy in STRATEGIES:
        r = device_sample(eng, g, starts, hops=4, strategy=strategy, seed=13)
        again = device_sample(eng, g, starts, hops=4, strategy=strategy,
                              seed=13)
        assert np.array_equal(r["paths"], again["paths"])
        assert np.array_equal(r["paths"][:, 0], starts)
        assert (r["paths"][:, -1] >= 0).sum() > 250
        for path in r["paths"]:
            for h in range(4):
                a, b = int(path[h]), int(path[h + 1])
                assert (a, b) in arcs if b >= 0 else True, (strategy, path)


def test_arbitrary_oids(eng):
    """Hash vertex map: the device ids are renumbered, the paths come back in
    oids and every step is an arc."""
    src, dst, w = simple_graph(False, num_v=500, arcs=6000, seed=251)
    rng = np.random.default_rng(252)
    oids = rng.choice(10 ** 12, size=500, replace=False).astype(np.int64)
    g = eng.load_edges(oids[src], oids[dst], weights=w, directed=False,
                       vertex_oids=oids, idxer="hashmap")
    arcs = set(zip(oids[src].tolist(), oids[dst].tolist()))
    arcs |= {(b, a) for a, b in arcs}
    starts = np.concatenate([oids[:200], [5, -7]])
    for strategy in STRATEGIES:
        r = device_sample(eng, g, starts, hops=3, strategy=strategy)
        assert np.array_equal(r["walk_ids"], np.arange(200))
        assert np.array_equal(r["paths"][:, 0], oids[:200])
        for path in r["paths"]:
            for h in range(3):
                if path[h + 1] >= 0:
                    assert (int(path[h]), int(path[h + 1])) in arcs


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
    r = eng.sample(g, d["starts"], hops=4, strategy=strategy, top_k=4, seed=7,
                   device=True)
    out[strategy] = {"walk_ids": r["walk_ids"].tolist(),
                     "paths": r["paths"].tolist(),
                     "rounds": int(r["rounds"]),
                     "steps": int(r["traversed_edges"]),
                     "bytes_p2p": int(r["bytes_p2p"])}
out["calls"] = int(eng._debug_sample()["calls"])
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
    starts = graph1_starts()
    graph_file = tmp_path / "graph.npz"
    np.savez(graph_file, src=src, dst=dst, w=w, starts=starts, num_v=2000)
    want = {s: walk_oracle(2000, src, dst, w, starts, 4, s, top_k=4, seed=7,
                           directed=False) for s in STRATEGIES}
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        slice_ = (2000 + world - 1) // world
        for s in STRATEGIES:
            # at least a third of the oracle's steps leave their slice
            p = want[s][1]
            moves = p[:, 1:] >= 0
            cross = moves & (p[:, :-1] // slice_ != p[:, 1:] // slice_)
            assert 3 * cross.sum() >= moves.sum() > 1000, (world, s)
        ranks = run_world(world, tmp_path / ("w%d" % world), pick_port(),
                          graph_file)
        for d in ranks:
            assert d["calls"] == 3  # every result came from the device
        for s in STRATEGIES:
            ids = np.concatenate([np.asarray(d[s]["walk_ids"], dtype=np.int64)
                                  for d in ranks])
            paths = np.concatenate(
                [np.asarray(d[s]["paths"], dtype=np.int64).reshape(-1, 5)
                 for d in ranks])
            # every walk on exactly one rank, with the oracle's path
            order = np.argsort(ids, kind="stable")
            assert np.array_equal(ids[order], want[s][0]), (world, s)
            assert np.array_equal(paths[order], want[s][1]), (world, s)
            for rank, d in enumerate(ranks):
                own = starts[np.asarray(d[s]["walk_ids"], dtype=np.int64)]
                assert ((own // slice_) == rank).all(), (world, s, rank)
                assert d[s]["rounds"] == 4
                assert d[s]["steps"] == int((want[s][1][:, 1:] >= 0).sum())
            assert sum(d[s]["bytes_p2p"] for d in ranks) > 0, (world, s)
            assert all(d[s]["bytes_p2p"] > 0 for d in ranks), (world, s)


# --- 9. CLI -----------------------------------------------------------------

@pytest.mark.parametrize("strategy", ("edge_weight", "top_k"))
def test_cli_sample(tmp_path, strategy):
    src, dst, w = simple_graph(True, num_v=200, arcs=1500, seed=261)
    efile = tmp_path / "g.e"
    with open(efile, "w") as f:
        for a, b, x in zip(src, dst, w):
            f.write("%d %d %s\n" % (a, b, repr(float(x))))
    out = tmp_path / "gpu"
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application",
           "sample", "--sample_walks", "150", "--sample_hops", "3",
           "--sample_strategy", strategy, "--sample_top_k", "3",
           "--sample_seed", "9", "--efile", str(efile), "--weighted",
           "--directed", "--vertex_num", "200", "--out_prefix", str(out),
           "--gpu"]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ids, paths = walk_oracle(200, src, dst, w, np.arange(150), 3, strategy,
                             top_k=3, seed=9)
    want = ["%d %s" % (i, " ".join(map(str, p))) for i, p in zip(ids, paths)]
    assert len(want) == 150
    assert open(out / "result_frag_0").read().splitlines() == want
