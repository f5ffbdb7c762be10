"""The four frontier schedulers (GRAPEHIP_LB=cm|wm|strict|none) under every
op that goes through them: BFS push, SSSP, the WCC rest pass, the CDLP
dirty-row marking and k-core peeling. Each run is compared exactly with the
oracles, and the engine's host-side launch counters prove that the scheduler
asked for is the one that ran. GRAPEHIP_LB and GRAPEHIP_BFS_PULL_DIV are read
once per process, so every configuration is a fresh child process; children
run strictly one after another."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracles import (DBL_MAX, INT64_MAX, bfs_oracle, cdlp_oracle_fast,
                     coreness_oracle_fast, sssp_oracle_f32, wcc_oracle)

REPO = Path(__file__).resolve().parent.parent

LBS = ("cm", "wm", "strict", "none")
CDLP_ITERS = 10

CHAIN = 50
STAR_LEAVES = 5001
HUB_LEAVES, HUB_PARALLEL = 400, 100     # 40,000 arcs in one row
LAYERS = (64, 256, 257)
N_COMMUNITIES = 250


def sched_graph():
    """One edge list, loaded directed (with in-CSR) and undirected. Arcs
    point away from the BFS/SSSP source, the head of the chain, and the
    gadgets hang on one another so that each has levels to itself:

    chain of 50 -> star hub -> 5001 star leaves -> (from one leaf) big hub
    -> 400 hub leaves -> (from 2 of them) layer of 64 -> 256 -> 257.

    - chain: a frontier of one entry for 50 levels (grids of one block, a
      wave with one live lane, strict with more blocks than arcs).
    - star hub: one entry of 5001 arcs; then the 5001 leaves. Undirected,
      they carry 5001 arcs back (78 waves + 9 lanes, 19 cm chunks + 137
      threads: the ragged last trip that once broke wm). Directed, all but
      one are sinks: whole waves and whole cm chunks without an arc, and the
      owner search crosses runs of equal prefixes.
    - big hub: 40,000 arcs (100 parallel arcs of different weights to each of
      400 leaves) as the only frontier entry: cm sweeps one chunk 157
      times, strict cuts the row over 157 blocks, none walks it in one
      thread. Directed, its leaves are sinks but every 300th: a run of 299
      queue entries of out-degree 0.
    - layers: complete bipartite, so the frontiers have exactly 64, 256 and
      257 entries (one wave, one cm chunk, one chunk plus one entry).
      Directed, the last layer is a frontier with no arc at all.
    - communities: 250 components of 100 to 500 vertices and mean degree 20,
      so the two arcs a row samples first do not join a component and the
      WCC rest pass has real work; planted communities let CDLP settle, so
      that fewer than 1/8 of the labels change and the dirty-row marking
      runs (stars, chains and bipartite layers flip their labels for ever:
      they are kept small against the communities for this reason).
    Undirected, WCC leaves out the largest component it probes, which is the
    gadget chain; directed, sinks keep the gadgets apart after sampling and
    the rest pass takes them all, in-arcs included.

    Returns (src, dst, w, num_v, source)."""
    rng = np.random.default_rng(41)
    nxt = 0

    def take(n):
        nonlocal nxt
        ids = np.arange(nxt, nxt + n, dtype=np.int64)
        nxt += n
        return ids

    chain, star_hub, star = take(CHAIN), take(1), take(STAR_LEAVES)
    hub, hub_leaves = take(1), take(HUB_LEAVES)
    la, lb, lc = (take(n) for n in LAYERS)
    src = [chain[:-1], chain[-1:], np.repeat(star_hub, STAR_LEAVES),
           star[2500:2501], np.repeat(hub, HUB_LEAVES * HUB_PARALLEL),
           np.repeat(hub_leaves[::300], len(la)), np.repeat(la, len(lb)),
           np.repeat(lb, len(lc))]
    dst = [chain[1:], star_hub, star, hub,
           np.tile(hub_leaves, HUB_PARALLEL),
           np.tile(la, len(hub_leaves[::300])), np.tile(lb, len(la)),
           np.tile(lc, len(lb))]
    for _ in range(N_COMMUNITIES):
        ids = take(int(rng.integers(100, 501)))
        a = rng.integers(0, len(ids), 10 * len(ids))
        b = rng.integers(0, len(ids), 10 * len(ids))
        keep = a != b
        src.append(ids[a[keep]])
        dst.append(ids[b[keep]])
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = (rng.random(len(src), dtype=np.float32) * 9 + 1).astype(np.float32)
    return src, dst, w, nxt, int(chain[0])


def wide_star():
    """Undirected star of 2048 * 256 + 300 leaves around vertex 0: the leaf
    frontier is one entry more than a full grid covers in one trip, plus a
    ragged tail, under every scheduler."""
    n = 2048 * 256 + 300
    rng = np.random.default_rng(43)
    src = np.zeros(n, dtype=np.int64)
    dst = np.arange(1, n + 1, dtype=np.int64)
    w = (rng.random(n, dtype=np.float32) * 9 + 1).astype(np.float32)
    return src, dst, w, n + 1


WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_schedulers import CDLP_ITERS, sched_graph, wide_star

mode = os.environ["GRAPEHIP_SCHED_MODE"]
eng = grapehip.Engine(rank=0, world=1, gpu=True)
out = {}

def run(tag, name, fn, arrays):
    before = eng._debug_expand_counts()
    r = fn()
    after = eng._debug_expand_counts()
    arrays[tag + "_" + name] = np.asarray(r["values"])[np.argsort(r["oids"])]
    out[tag + "_" + name + "_counts"] = {k: after[k] - before[k]
                                         for k in after}

if mode == "wide":
    src, dst, w, num_v = wide_star()
    g = eng.load_edges(src, dst, weights=w, directed=False,
                       num_vertices=num_v)
    arrays = {}
    run("wide", "bfs", lambda: eng.bfs(g, 1), arrays)
    run("wide", "sssp", lambda: eng.sssp(g, 1), arrays)
    run("wide", "wcc", lambda: eng.wcc(g), arrays)
    # half a million values per app: as an array file, not as JSON text
    np.savez(os.environ["GRAPEHIP_OUT"], **arrays)
else:
    src, dst, w, num_v, source = sched_graph()
    for tag, directed in (("dir", True), ("und", False)):
        g = eng.load_edges(src, dst, weights=w, directed=directed,
                           num_vertices=num_v, build_in_csr=directed)
        arrays = {}
        run(tag, "bfs", lambda: eng.bfs(g, source), arrays)
        if mode == "all":
            run(tag, "sssp", lambda: eng.sssp(g, source), arrays)
            run(tag, "wcc", lambda: eng.wcc(g), arrays)
            run(tag, "cdlp", lambda: eng.cdlp(g, CDLP_ITERS), arrays)
            run(tag, "core", lambda: eng.core_decomposition(g), arrays)
        for k, v in arrays.items():
            out[k] = v.tolist()
print("RESULT " + json.dumps(out))
'''


def run_child(lb, pull_div, mode, out=None):
    env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_LB=lb,
               GRAPEHIP_BFS_PULL_DIV=str(pull_div), GRAPEHIP_SCHED_MODE=mode)
    if out is not None:
        env["GRAPEHIP_OUT"] = str(out)
    r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                       capture_output=True, text=True, timeout=120)
    # a child that died stops the test here: nothing else is launched
    assert r.returncode == 0, (lb, r.stdout[-2000:] + r.stderr[-2000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert len(line) == 1, (lb, r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(line[0][len("RESULT "):])


def assert_only(counts, lb, what):
    assert counts[lb] > 0, (what, counts)
    for other in LBS:
        if other != lb:
            assert counts[other] == 0, (what, counts)


def assert_same_partition(got, exp):
    fwd, bwd = {}, {}
    for a, b in zip(got.tolist(), exp.tolist()):
        assert fwd.setdefault(a, b) == b
        assert bwd.setdefault(b, a) == a


def assert_sssp_exact(got, exp):
    got = np.asarray(got, dtype=np.float64)
    unreached = exp > 1e300
    assert np.array_equal(got > 1e300, unreached)
    assert np.array_equal(got[~unreached].astype(np.float32),
                          exp[~unreached].astype(np.float32))


@functools.lru_cache(maxsize=None)
def expected():
    """Oracle results for sched_graph, computed once for the module."""
    src, dst, w, num_v, source = sched_graph()
    exp = {}
    for tag, directed in (("dir", True), ("und", False)):
        exp[tag + "_bfs"] = bfs_oracle(num_v, src, dst, source,
                                       directed=directed)
        exp[tag + "_sssp"] = sssp_oracle_f32(num_v, src, dst, w, source,
                                             directed=directed)
        exp[tag + "_core"] = coreness_oracle_fast(num_v, src, dst,
                                                  directed=directed)
    wcc = wcc_oracle(num_v, src, dst)
    cdlp, changed = cdlp_oracle_fast(num_v, src, dst, CDLP_ITERS,
                                     return_changed=True)
    for tag in ("dir", "und"):
        exp[tag + "_wcc"], exp[tag + "_cdlp"] = wcc, cdlp
    return exp, changed, num_v


def test_graph_has_the_shapes():
    # conditions the GPU cases rely on, checked from the oracles alone
    src, dst, w, num_v, source = sched_graph()
    exp, changed, _ = expected()
    assert 20000 < num_v < 90000
    for tag in ("dir", "und"):
        depth = exp[tag + "_bfs"]
        sizes = np.bincount(depth[depth < INT64_MAX])
        # chain, star hub, star leaves, big hub, its leaves, three layers
        assert sizes.tolist() == ([1] * (CHAIN + 1) + [STAR_LEAVES, 1,
                                                       HUB_LEAVES]
                                  + list(LAYERS))
    outdeg = np.bincount(src, minlength=num_v)
    assert outdeg.max() == HUB_LEAVES * HUB_PARALLEL
    star = np.flatnonzero(exp["dir_bfs"] == CHAIN + 1)
    assert (outdeg[star] == 0).sum() == STAR_LEAVES - 1
    leaves = np.flatnonzero(exp["dir_bfs"] == CHAIN + 3)
    assert (outdeg[leaves] == 0).sum() == HUB_LEAVES - 2
    assert (outdeg[leaves[1:300]] == 0).all()   # a run of 299 > 256 sinks
    # no component but the gadget chain is large
    comp = np.bincount(np.unique(exp["und_wcc"], return_inverse=True)[1])
    assert len(comp) >= N_COMMUNITIES + 1 and np.sort(comp)[-2] <= 500
    # CDLP: some iteration before the last changes labels, but fewer than
    # 1/8 of them, so the next one expands the changed rows
    assert any(0 < c < num_v // 8 for c in changed[:-1]), changed


@pytest.mark.gpu
@pytest.mark.parametrize("lb", LBS)
def test_scheduler_runs_and_is_exact(lb):
    exp, _, num_v = expected()
    # threshold = all stored arcs, which no frontier exceeds: always push
    got = run_child(lb, 1, "all")
    for tag in ("dir", "und"):
        for app in ("bfs", "sssp", "wcc", "cdlp", "core"):
            name = tag + "_" + app
            assert_only(got[name + "_counts"], lb, name)
            vals = np.asarray(got[name])
            assert len(vals) == num_v
            if app == "sssp":
                assert_sssp_exact(vals, exp[name])
            elif app == "wcc":
                assert_same_partition(vals, exp[name])
            else:
                assert np.array_equal(vals, exp[name]), name


@pytest.mark.gpu
def test_bfs_pull_at_every_level():
    exp, _, _ = expected()
    # threshold 0: every level whose frontier has an arc pulls
    got = run_child("cm", 1000000000, "pull")
    for tag in ("dir", "und"):
        assert np.array_equal(np.asarray(got[tag + "_bfs"]),
                              exp[tag + "_bfs"]), tag
        # levels without a frontier arc (directed: the last layer) still
        # push; the chain alone gives the undirected graph 50 pulls
        counts = got[tag + "_bfs_counts"]
        assert sum(counts.values()) == (1 if tag == "dir" else 0), counts


@pytest.mark.gpu
@pytest.mark.parametrize("lb", LBS)
def test_grid_stride_trip(lb, tmp_path):
    src, dst, w, num_v = wide_star()
    assert num_v - 1 > 2048 * 256
    out = tmp_path / "wide.npz"
    got = run_child(lb, 1, "wide", out)
    arrays = np.load(out)
    depth = np.full(num_v, 2, dtype=np.int64)
    depth[0], depth[1] = 1, 0
    assert np.array_equal(arrays["wide_bfs"], depth)
    dist = (w[0] + w).astype(np.float32)      # leaf j: fp32(w_1 + w_j)
    assert dist.dtype == np.float32
    dist = np.concatenate([[w[0]], dist]).astype(np.float32)
    dist[1] = 0.0
    assert np.array_equal(arrays["wide_sssp"].astype(np.float32), dist)
    assert (arrays["wide_sssp"] < 1e300).all()
    assert (arrays["wide_wcc"] == arrays["wide_wcc"][0]).all()
    for app in ("bfs", "sssp"):
        assert_only(got["wide_%s_counts" % app], lb, app)
    # sampling alone joins a star, so the WCC rest pass may have no row left
    wcc = got["wide_wcc_counts"]
    assert all(wcc[other] == 0 for other in LBS if other != lb), wcc
