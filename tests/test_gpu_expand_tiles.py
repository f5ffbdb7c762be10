"""The default (cm) frontier expansion cuts the frontier's arc space into
tiles of GRAPEHIP_EXPAND_TILE arcs. These tests force tiles of a few hundred
arcs, so that small graphs put tile edges inside rows, on row edges, inside
runs of entries without an arc, over more than 256 owners and past the grid
cap, and compare every app that expands frontiers exactly with the oracles.
k-core subtracts once per arc, so its exact coreness is the check that every
arc is handed out exactly once (BFS and SSSP would hide a second visit).

The workspace test runs BFS and SSSP on graphs of different sizes in one
engine: the device buffers are kept across calls and a smaller graph uses a
prefix of them.

GRAPEHIP_EXPAND_TILE is read once per process, so every configuration is a
fresh child process; children run strictly one after another, each under its
own timeout."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracles import bfs_oracle, coreness_oracle_fast, sssp_oracle_f32
from test_gpu_schedulers import (LBS, assert_only, assert_same_partition,
                                 assert_sssp_exact, expected, wide_star)

REPO = Path(__file__).resolve().parent.parent

ALIGN_DEGREES = (256, 0, 0, 256, 1, 255, 512)


def align_graph():
    """Source 0 -> vertices 1..7 -> a pool of 512 vertices (8..519). Loaded
    directed, vertices 1..7 have out-degrees ALIGN_DEGREES and form BFS level
    1 and, with every weight below delta, one SSSP near frontier. The queue
    order is the id order: compact_frontier emits ascending device ids, and a
    host-loaded graph with num_vertices given keeps its ids (no renumbering;
    the worker asserts that the rows come back as 0..n-1). The prefix is
    [0, 256, 256, 256, 512, 513, 768, 1280]: with tiles of 256 arcs, tile 1
    starts behind the run of two entries without an arc, tiles 2 and 3 start
    on row edges and tile 4 inside the last row. The pool vertices are sinks:
    the next frontier has no arc. The undirected load of the same arcs gives
    every level-1 row one arc more (back to the source; an undirected
    frontier cannot hold a row without an arc), so there no tile edge is
    aligned.

    Returns (src, dst, w, num_v, source)."""
    rng = np.random.default_rng(47)
    pool = np.arange(8, 8 + 512, dtype=np.int64)
    picks = {1: pool[:256], 4: pool[256:], 5: pool[300:301], 6: pool[1:256],
             7: pool}
    src = [np.zeros(7, dtype=np.int64)]
    dst = [np.arange(1, 8, dtype=np.int64)]
    for v, nbrs in picks.items():
        src.append(np.full(len(nbrs), v, dtype=np.int64))
        dst.append(nbrs)
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = (rng.random(len(src), dtype=np.float32) * 9 + 1).astype(np.float32)
    return src, dst, w, 8 + 512, 0


def reuse_graphs():
    """(large, small): random graphs of 30,000 and 1,000 vertices with
    (src, dst, w, num_v)."""
    out = []
    for seed, num_v, ne in ((51, 30000, 150000), (53, 1000, 4000)):
        rng = np.random.default_rng(seed)
        src = rng.integers(0, num_v, ne)
        dst = rng.integers(0, num_v, ne)
        w = (rng.random(ne, dtype=np.float32) * 9 + 1).astype(np.float32)
        out.append((src, dst, w, num_v))
    return out


# (graph index, source) in call order: large, small, large again
REUSE_CALLS = ((0, 3), (1, 7), (0, 3), (0, 11), (1, 0))


WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_schedulers import CDLP_ITERS, sched_graph, wide_star
from test_gpu_expand_tiles import REUSE_CALLS, align_graph, reuse_graphs

mode = os.environ["GRAPEHIP_TILE_MODE"]
eng = grapehip.Engine(rank=0, world=1, gpu=True)
out = {}
arrays = {}

def run(name, fn):
    before = eng._debug_expand_counts()
    r = fn()
    after = eng._debug_expand_counts()
    arrays[name] = np.asarray(r["values"])[np.argsort(r["oids"])]
    out[name + "_counts"] = {k: after[k] - before[k] for k in after}
    return r

if mode == "sched":
    src, dst, w, num_v, source = sched_graph()
    for tag, directed in (("dir", True), ("und", False)):
        g = eng.load_edges(src, dst, weights=w, directed=directed,
                           num_vertices=num_v, build_in_csr=directed)
        run(tag + "_bfs", lambda: eng.bfs(g, source))
        run(tag + "_sssp", lambda: eng.sssp(g, source))
        run(tag + "_wcc", lambda: eng.wcc(g))
        run(tag + "_cdlp", lambda: eng.cdlp(g, CDLP_ITERS))
        run(tag + "_core", lambda: eng.core_decomposition(g))
elif mode == "wide":
    src, dst, w, num_v = wide_star()
    g = eng.load_edges(src, dst, weights=w, directed=False,
                       num_vertices=num_v)
    run("wide_bfs", lambda: eng.bfs(g, 1))
    run("wide_sssp", lambda: eng.sssp(g, 1))
    run("wide_core", lambda: eng.core_decomposition(g))
elif mode == "align":
    src, dst, w, num_v, source = align_graph()
    for tag, directed in (("dir", True), ("und", False)):
        g = eng.load_edges(src, dst, weights=w, directed=directed,
                           num_vertices=num_v, build_in_csr=directed)
        r = run(tag + "_bfs", lambda: eng.bfs(g, source))
        # rows come back in upload order: device id == vertex id
        assert np.array_equal(np.asarray(r["oids"]), np.arange(num_v))
        run(tag + "_sssp", lambda: eng.sssp(g, source))
        run(tag + "_core", lambda: eng.core_decomposition(g))
elif mode == "reuse":
    graphs = [eng.load_edges(s, d, weights=w, directed=False, num_vertices=n)
              for s, d, w, n in reuse_graphs()]
    for i, (gi, source) in enumerate(REUSE_CALLS):
        run("bfs%d" % i, lambda: eng.bfs(graphs[gi], source, values=True))
        run("sssp%d" % i, lambda: eng.sssp(graphs[gi], source, values=True))
np.savez(os.environ["GRAPEHIP_OUT"], **arrays)
print("RESULT " + json.dumps(out))
'''


def run_child(tile, mode, out):
    env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_TILE_MODE=mode,
               GRAPEHIP_OUT=str(out),
               # threshold = all stored arcs, which no frontier exceeds: BFS
               # always pushes
               GRAPEHIP_BFS_PULL_DIV="1")
    env.pop("GRAPEHIP_LB", None)            # the default scheduler
    env.pop("GRAPEHIP_EXPAND_TILE", None)
    if tile is not None:
        env["GRAPEHIP_EXPAND_TILE"] = str(tile)
    r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                       capture_output=True, text=True, timeout=120)
    # a child that died stops the test here: nothing else is launched
    assert r.returncode == 0, (tile, r.stdout[-2000:] + r.stderr[-2000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert len(line) == 1, (tile, r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(line[0][len("RESULT "):]), np.load(out)


def assert_only_cm(counts, what):
    for name, c in counts.items():
        assert all(c[lb] == 0 for lb in LBS if lb != "cm"), (what, name, c)


@functools.lru_cache(maxsize=None)
def align_expected():
    src, dst, w, num_v, source = align_graph()
    exp = {}
    for tag, directed in (("dir", True), ("und", False)):
        exp[tag + "_bfs"] = bfs_oracle(num_v, src, dst, source,
                                       directed=directed)
        exp[tag + "_sssp"] = sssp_oracle_f32(num_v, src, dst, w, source,
                                             directed=directed)
        exp[tag + "_core"] = coreness_oracle_fast(num_v, src, dst,
                                                  directed=directed)
    return exp


def test_align_graph_has_the_shape():
    # what the GPU case relies on, checked from the edge list alone
    src, dst, w, num_v, source = align_graph()
    outdeg = np.bincount(src, minlength=num_v)
    assert outdeg[1:8].tolist() == list(ALIGN_DEGREES)
    assert (outdeg[8:] == 0).all()
    prefix = np.concatenate([[0], np.cumsum(ALIGN_DEGREES)])
    assert prefix.tolist() == [0, 256, 256, 256, 512, 513, 768, 1280]
    depth = align_expected()["dir_bfs"]
    assert np.flatnonzero(depth == 1).tolist() == list(range(1, 8))
    # one SSSP near frontier: the default delta is 16 mean weights, far
    # above any single weight
    assert w.max() < 10 < 16 * w.mean()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", (256, 512))
def test_exact_under_small_tiles(tile, tmp_path):
    exp, _, num_v = expected()
    counts, got = run_child(tile, "sched", tmp_path / "sched.npz")
    for tag in ("dir", "und"):
        for app in ("bfs", "sssp", "wcc", "cdlp", "core"):
            name = tag + "_" + app
            assert_only(counts[name + "_counts"], "cm", name)
            vals = got[name]
            assert len(vals) == num_v
            if app == "sssp":
                assert_sssp_exact(vals, exp[name])
            elif app == "wcc":
                assert_same_partition(vals, exp[name])
            else:
                assert np.array_equal(vals, exp[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("tile", (256, 1024))
def test_tiles_over_many_owners(tile, tmp_path):
    src, dst, w, num_v = wide_star()
    # leaf frontier of entries with one arc each: more tiles of 256 than the
    # grid cap of 2048; a tile of 1024 stages four batches of 256 owners
    assert (num_v - 2 + 255) // 256 > 2048
    counts, got = run_child(tile, "wide", tmp_path / "wide.npz")
    depth = np.full(num_v, 2, dtype=np.int64)
    depth[0], depth[1] = 1, 0
    assert np.array_equal(got["wide_bfs"], depth)
    dist = np.concatenate([[w[0]], (w[0] + w).astype(np.float32)])
    dist = dist.astype(np.float32)            # leaf j: fp32(w_1 + w_j)
    dist[1] = 0.0
    assert (got["wide_sssp"] < 1e300).all()
    assert np.array_equal(got["wide_sssp"].astype(np.float32), dist)
    assert np.array_equal(got["wide_core"],
                          coreness_oracle_fast(num_v, src, dst))
    for app in ("bfs", "sssp", "core"):
        assert_only(counts["wide_%s_counts" % app], "cm", app)


@pytest.mark.gpu
def test_tile_edges_on_row_edges(tmp_path):
    exp = align_expected()
    counts, got = run_child(256, "align", tmp_path / "align.npz")
    for tag in ("dir", "und"):
        assert np.array_equal(got[tag + "_bfs"], exp[tag + "_bfs"]), tag
        assert_sssp_exact(got[tag + "_sssp"], exp[tag + "_sssp"])
        assert np.array_equal(got[tag + "_core"], exp[tag + "_core"]), tag
    assert_only_cm(counts, "align")


@pytest.mark.gpu
def test_workspace_reuse(tmp_path):
    graphs = reuse_graphs()
    counts, got = run_child(None, "reuse", tmp_path / "reuse.npz")
    for i, (gi, source) in enumerate(REUSE_CALLS):
        src, dst, w, num_v = graphs[gi]
        assert np.array_equal(
            got["bfs%d" % i],
            bfs_oracle(num_v, src, dst, source, directed=False)), i
        assert_sssp_exact(
            got["sssp%d" % i],
            sssp_oracle_f32(num_v, src, dst, w, source, directed=False))
    # calls 0 and 2: the larger graph before and after the smaller one
    assert REUSE_CALLS[0] == REUSE_CALLS[2]
    assert np.array_equal(got["bfs0"], got["bfs2"])
    assert np.array_equal(got["sssp0"], got["sssp2"])
    assert_only_cm(counts, "reuse")
