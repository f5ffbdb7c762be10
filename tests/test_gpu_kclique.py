"""GPU k-clique counting (bitmap enumeration over the oriented CSR) on one
MI355X: the HIP path vs the recursive oracle and the dense oracle, closed
forms, the three row tiers and their boundaries, arbitrary oids, a
device-only graph, the host engine, worlds 2 and 4 over the TCP-staged data
plane and the CLI. Counts are integers, so every comparison is exact.

Every test that calls the device asserts that the `_debug_kclique` call
counter went up: without the device path the hook does not exist and the
count would come from the host app."""
import json
import os
import subprocess
import sys
from math import comb
from pathlib import Path

import numpy as np
import pytest

import grapehip
from oracles import kclique_oracle, lcc_oracle
from test_gpu_kcore import multigraph, pick_port
from test_kclique_dense_oracle import (dense_adjacency, gnp_upper,
                                       kclique_dense)

REPO = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29731, gpu=True)


def device_count(eng, g, k):
    """kclique on the device: the call counter must move."""
    before = eng._debug_kclique()["calls"]
    r = eng.kclique(g, k)
    assert eng._debug_kclique()["calls"] == before + 1, k
    assert "oids" not in r and "values" not in r
    for key in ("rounds", "seconds", "traversed_edges", "bytes_p2p",
                "bytes_coll"):
        assert key in r, key
    assert r["rounds"] == 1
    return int(r["clique_count"])


def complete_graph(n, base=0):
    src, dst = np.nonzero(np.triu(np.ones((n, n), dtype=bool), 1))
    return src.astype(np.int64) + base, dst.astype(np.int64) + base


def oriented_degrees(num_v, src, dst):
    """|O(v)| of the (degree, id) orientation on the simple graph."""
    A = dense_adjacency(num_v, src, dst)
    key = A.sum(1).astype(np.int64) * num_v + np.arange(num_v)
    return (A & (key[None, :] > key[:, None])).sum(1)


# --- 1. oracle, random undirected multigraph -------------------------------

def test_oracle_random_multigraph(eng):
    src, dst = multigraph(num_v=120, num_e=1500, loops=10, seed=101)
    g = eng.load_edges(src, dst, directed=False, num_vertices=120)
    for k in range(2, 7):
        assert device_count(eng, g, k) == kclique_oracle(120, src, dst, k), k


# --- 2. closed forms --------------------------------------------------------

N_LEAVES = 5000
BIP = 40
PATH = 10
ISOLATED = 7
CLIQUE = 12


def shapes_graph():
    """Star of 5000 leaves, K_{40,40}, a 10-path, 7 isolated vertices, a pair
    joined by three parallel edges and a disjoint K_12.
    Returns (src, dst, num_v, {k: expected count})."""
    src, dst = [], []
    src += [0] * N_LEAVES
    dst += list(range(1, N_LEAVES + 1))
    base = N_LEAVES + 1
    for i in range(BIP):
        for j in range(BIP):
            src.append(base + i)
            dst.append(base + BIP + j)
    base += 2 * BIP
    for i in range(PATH - 1):
        src.append(base + i)
        dst.append(base + i + 1)
    base += PATH + ISOLATED
    src += [base] * 3
    dst += [base + 1] * 3
    base += 2
    cs, cd = complete_graph(CLIQUE, base)
    base += CLIQUE
    edges = N_LEAVES + BIP * BIP + (PATH - 1) + 1
    expect = {2: edges + comb(CLIQUE, 2)}
    for k in (3, 4, 5):  # star, bipartite, path and pair hold no triangle
        expect[k] = comb(CLIQUE, k)
    return (np.concatenate([np.array(src, dtype=np.int64), cs]),
            np.concatenate([np.array(dst, dtype=np.int64), cd]), base, expect)


def test_closed_form_shapes(eng):
    src, dst, num_v, expect = shapes_graph()
    g = eng.load_edges(src, dst, directed=False, num_vertices=num_v)
    for k in (2, 3, 4, 5):
        assert device_count(eng, g, k) == expect[k], k


@pytest.mark.parametrize("n", (3, 64, 65, 66))
def test_complete_graph_wave_boundary(eng, n):
    src, dst = complete_graph(n)
    g = eng.load_edges(src, dst, directed=False, num_vertices=n)
    for k in (3, 4, 5):
        assert device_count(eng, g, k) == comb(n, k), (n, k)
        hook = eng._debug_kclique()
        # vertex 0 has the longest oriented row, n - 1 entries: the block
        # tier starts at 65
        assert hook["rows_block"] == (1 if n == 66 else 0), (n, k)
        assert hook["rows_global"] == 0


# --- 3. tiers ---------------------------------------------------------------

def test_block_tier_gnp(eng):
    src, dst = gnp_upper(150, 0.7, seed=5)
    assert len(src) == 7856
    od = oriented_degrees(150, src, dst)
    assert od.max() == 93 and (od > 64).sum() == 60
    A = dense_adjacency(150, src, dst)
    g = eng.load_edges(src, dst, directed=False, num_vertices=150)
    for k in (3, 4):
        assert device_count(eng, g, k) == kclique_dense(A, k), k
        hook = eng._debug_kclique()
        assert hook["rows_block"] == 60 and hook["rows_global"] == 0


def test_global_tier_gnp(eng):
    block_max = eng._debug_kclique()["block_max"]
    n = int(1.4 * block_max)
    src, dst = gnp_upper(n, 0.85, seed=5)
    od = oriented_degrees(n, src, dst)
    n_global = int((od > block_max).sum())
    assert n_global > 0  # before any GPU call: the draw reaches the tier
    if block_max == 512:
        assert (n, len(src), n_global) == (716, 217675, 107)
    A = dense_adjacency(n, src, dst)
    g = eng.load_edges(src, dst, directed=False, num_vertices=n)
    for k in ((3, 4) if n <= 800 else (3,)):
        want = kclique_dense(A, k)
        if block_max == 512:
            assert want == {3: 37465177, 4: 4106997800}[k]
        assert device_count(eng, g, k) == want, k
        hook = eng._debug_kclique()
        assert hook["rows_global"] == n_global
        assert hook["rows_block"] == int(((od > 64) & (od <= block_max)).sum())


def test_global_tier_complete_graph(eng):
    n = eng._debug_kclique()["block_max"] + 2
    src, dst = complete_graph(n)
    g = eng.load_edges(src, dst, directed=False, num_vertices=n)
    for k in (3, 4):
        assert device_count(eng, g, k) == comb(n, k), k  # C(n, 4) > 2^31
        assert eng._debug_kclique()["rows_global"] == 1


# --- 4. arbitrary oids (hashmap idxer, padded owned range) -----------------

def test_arbitrary_oids(eng):
    si, di = multigraph(num_v=500, num_e=6000, loops=20, seed=103)
    rng = np.random.default_rng(104)
    oids = rng.choice(10**12, size=500, replace=False).astype(np.int64)
    g = eng.load_edges(oids[si], oids[di], directed=False, vertex_oids=oids,
                       idxer="hashmap")
    gi = eng.load_edges(si, di, directed=False, num_vertices=500)
    for k in (2, 3, 4):
        want = kclique_oracle(500, si, di, k)
        assert device_count(eng, gi, k) == want, k
        assert device_count(eng, g, k) == want, k


# --- 5. device-only graph, limits, host engine -----------------------------

@pytest.fixture(scope="module")
def synthetic(eng):
    return eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7)


def test_device_only_graph_runs(eng, synthetic):
    # no host fragment: the host app cannot run on this graph at all
    arcs = device_count(eng, synthetic, 2)
    assert 0 < arcs <= 160000
    c3, c4 = device_count(eng, synthetic, 3), device_count(eng, synthetic, 4)
    assert c3 > 0 and c4 > 0
    assert eng.kclique(synthetic, 3)["traversed_edges"] == 160000


def test_limits_raise(eng, synthetic):
    k_max = eng._debug_kclique()["k_max"]
    assert k_max >= 8
    with pytest.raises(RuntimeError, match=str(k_max)):
        eng.kclique(synthetic, k_max + 1)
    with pytest.raises(RuntimeError, match="k must be >= 2"):
        eng.kclique(synthetic, 1)


def test_gpu_equals_host_rmat(eng):
    """GPU against the host app on RMAT edges of the size of the synthetic
    graph, loaded into both engines (as test_gpu_kcore does): 2^15 x 5 arcs
    folded into 20,000 vertices. The synthetic graph itself is counted
    against kclique_oracle in tests/test_gpu_synthetic_oracle.py, which
    models the generator's edges on the host."""
    src, dst, _, _ = grapehip.rmat_edges(15, edge_factor=5, seed=97)
    src, dst = src[:160000] % 20000, dst[:160000] % 20000
    cpu = grapehip.Engine(rank=0, world=1, master_port=29732)
    gc = cpu.load_edges(src, dst, directed=False, num_vertices=20000)
    gg = eng.load_edges(src, dst, directed=False, num_vertices=20000)
    for k in (3, 4):
        assert (device_count(eng, gg, k) ==
                int(cpu.kclique(gc, k)["clique_count"])), k


def test_above_k_max_uses_host_fragment(eng):
    k_max = eng._debug_kclique()["k_max"]
    src, dst = complete_graph(k_max + 3)
    g = eng.load_edges(src, dst, directed=False, num_vertices=k_max + 3)
    before = eng._debug_kclique()["calls"]
    r = eng.kclique(g, k_max + 1)
    assert r["clique_count"] == comb(k_max + 3, k_max + 1)
    assert eng._debug_kclique()["calls"] == before  # the host app ran
    assert device_count(eng, g, k_max) == comb(k_max + 3, k_max)


# --- 6. multi-rank over the TCP-staged data plane ---------------------------

MULTI_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
import grapehip
eng = grapehip.engine_from_env(gpu=True)
g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7)
out = {}
for k in (3, 4):
    r = eng.kclique(g, k)
    out[str(k)] = {"count": int(r["clique_count"]),
                   "bytes_p2p": int(r["bytes_p2p"])}
out["calls"] = int(eng._debug_kclique()["calls"])
path = os.path.join(os.environ["GRAPEHIP_OUT"],
                    "rank%s.json" % os.environ["RANK"])
json.dump(out, open(path, "w"))
'''


def run_world(world, outdir, port):
    outdir.mkdir()
    procs = []
    for rank in range(world):
        # every rank on device 0: the ranks stage payloads through TCP
        env = dict(os.environ, GRAPEHIP_REPO=str(REPO),
                   GRAPEHIP_OUT=str(outdir), RANK=str(rank), LOCAL_RANK="0",
                   WORLD_SIZE=str(world), GRAPEHIP_DATAPLANE="tcp",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
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
    ranks = [json.load(open(outdir / ("rank%d.json" % rank)))
             for rank in range(world)]
    for d in ranks:
        assert d["calls"] == 2  # both counts came from the device
    counts = {k: [d[str(k)]["count"] for d in ranks] for k in (3, 4)}
    sent = sum(d[str(k)]["bytes_p2p"] for d in ranks for k in (3, 4))
    return counts, sent


def test_multirank_matches_single(tmp_path, free_port):
    single, sent = run_world(1, tmp_path / "w1", free_port)
    assert sent == 0
    assert single[3][0] > 0 and single[4][0] > 0
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        got, sent = run_world(world, tmp_path / ("w%d" % world), pick_port())
        assert sent > 0, world  # oriented rows were fetched from their owners
        for k in (3, 4):
            assert got[k] == single[k] * world, (world, k)


# --- 7. CLI -----------------------------------------------------------------

def test_cli_kclique(tmp_path):
    rng = np.random.default_rng(105)
    nv = 200
    si = rng.integers(0, nv, 3000)
    di = rng.integers(0, nv, 3000)
    efile = tmp_path / "g.e"
    with open(efile, "w") as f:
        for a, b in zip(si, di):
            f.write("%d %d\n" % (a, b))
    out = tmp_path / "gpu"
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application",
           "kclique", "--kclique_k", "4", "--efile", str(efile),
           "--vertex_num", str(nv), "--out_prefix", str(out), "--gpu"]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = kclique_oracle(nv, si, di, 4)
    assert want > 0
    assert ("clique_num = %d" % want) in r.stdout.splitlines()
    assert open(out / "result_frag_0").read().split() == [str(want)]


# --- 8. repeatability, and no state left in the shared CSR helper ----------

def test_repeat_then_lcc(eng):
    src, dst = multigraph(num_v=400, num_e=6000, loops=15, seed=107)
    g = eng.load_edges(src, dst, directed=False, num_vertices=400)
    want = kclique_oracle(400, src, dst, 3)
    assert device_count(eng, g, 3) == want
    assert device_count(eng, g, 3) == want
    r = eng.lcc(g)
    got = np.asarray(r["values"])[np.argsort(r["oids"])]
    assert np.allclose(got, lcc_oracle(400, src, dst, directed=False),
                       rtol=1e-12)
    assert device_count(eng, g, 4) == kclique_oracle(400, src, dst, 4)
