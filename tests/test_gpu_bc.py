"""GPU betweenness centrality (single-source Brandes) on one MI355X: the HIP
path vs the NumPy oracle, closed-form shapes, the host engine, worlds 2 and 4
over the TCP-staged data plane, the four GRAPEHIP_LB schedulers and the CLI.

depth and path_num are compared exactly (every input keeps the path counts
below 2^53, asserted on the expectation first); values with
np.allclose(rtol=1e-9, atol=1e-9), the tolerance tests/test_cpu_apps.py holds
the host app to: the dependency sums add positive terms in an order the
device does not fix, which costs a few ulp."""
import json
import os
import socket
import subprocess
import sys
from math import comb
from pathlib import Path

import numpy as np
import pytest

import grapehip
from oracles import bc_oracle

REPO = Path(__file__).resolve().parent.parent
INT64_MAX = np.iinfo(np.int64).max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29731, gpu=True)


def by_oid(res, key="values"):
    order = np.argsort(res["oids"])
    return np.asarray(res[key])[order]


def oracle(num_v, src, dst, source, directed):
    """bc_oracle with the engine's conventions for unreached vertices."""
    delta, sigma, depth = bc_oracle(num_v, src, dst, source,
                                    directed=directed)
    reach = np.isfinite(depth)
    d64 = np.full(num_v, INT64_MAX, dtype=np.int64)
    d64[reach] = depth[reach].astype(np.int64)
    assert not delta[~reach].any() and not sigma[~reach].any()
    return delta, sigma, d64


def assert_bc(got_delta, got_sigma, got_depth, expect, tag=""):
    delta, sigma, depth = expect
    assert sigma.max() < 2.0 ** 53, tag  # path counts are exact integers
    err = np.abs(got_delta - delta)
    print("%s max |delta err| %.3e (max delta %.6e), reached %d of %d" %
          (tag, err.max(), delta.max(), int((depth != INT64_MAX).sum()),
           len(depth)))
    assert np.array_equal(got_depth, depth), tag
    assert np.array_equal(got_sigma, sigma), tag
    assert np.allclose(got_delta, delta, rtol=1e-9, atol=1e-9), tag


def assert_result(r, expect, tag=""):
    assert np.array_equal(np.sort(r["oids"]), np.arange(len(expect[0]))), tag
    assert_bc(by_oid(r), by_oid(r, "path_num"), by_oid(r, "depth"), expect,
              tag)


# --- 1. oracle, undirected multigraphs --------------------------------------

def test_oracle_undirected_multigraph(eng):
    rng = np.random.default_rng(91)
    src = rng.integers(0, 500, size=4000, dtype=np.int64)
    dst = rng.integers(0, 500, size=4000, dtype=np.int64)
    assert len(set(zip(src.tolist(), dst.tolist()))) < 4000  # duplicates
    expect = oracle(500, src, dst, 5, directed=False)
    assert (expect[2] != INT64_MAX).all() and expect[2].max() == 4
    g = eng.load_edges(src, dst, directed=False, num_vertices=500)
    r = eng.bc(g, 5)
    assert_result(r, expect, "dense")
    assert r["rounds"] == 5  # levels 0..4

    # sparse: many levels, thin frontiers and an unreached remainder
    rng = np.random.default_rng(95)
    src = rng.integers(0, 2000, size=2600, dtype=np.int64)
    dst = rng.integers(0, 2000, size=2600, dtype=np.int64)
    source = int(src[0])
    expect = oracle(2000, src, dst, source, directed=False)
    reach = expect[2] != INT64_MAX
    assert reach.sum() >= 0.85 * 2000 and not reach.all()
    assert expect[2][reach].max() >= 8
    g = eng.load_edges(src, dst, directed=False, num_vertices=2000)
    assert_result(eng.bc(g, source), expect, "sparse")


# --- 2. closed forms in one graph -------------------------------------------

N_LEAVES = 5000
DIAMONDS = 40
GRID = 24
PATH = 10
ISOLATED = 7


def shapes_graph():
    """Disjoint components: a star (hub row of 5000 arcs: crosses a 4096-arc
    tile and many 256-thread chunks), a chain of 40 diamonds, a 24x24 grid,
    a 10-vertex path, 7 isolated vertices and a pair joined by three
    parallel edges. Returns (src, dst, num_v, cases); a case is
    (name, source, {vertex: (delta, sigma, depth)}) and every vertex it
    leaves out is unreached from that source."""
    src, dst, cases = [], [], []

    hub, leaf0 = 0, 1
    src += [hub] * N_LEAVES
    dst += list(range(leaf0, leaf0 + N_LEAVES))
    from_leaf = {leaf0: (float(N_LEAVES), 1.0, 0),
                 hub: (float(N_LEAVES - 1), 1.0, 1)}
    from_hub = {hub: (float(N_LEAVES), 1.0, 0)}
    for v in range(leaf0, leaf0 + N_LEAVES):
        from_hub[v] = (0.0, 1.0, 1)
        if v != leaf0:
            from_leaf[v] = (0.0, 1.0, 2)
    cases += [("star from a leaf", leaf0, from_leaf),
              ("star from the hub", hub, from_hub)]
    base = leaf0 + N_LEAVES

    # diamonds: a_k - {b_k, c_k} - a_{k+1}; from a_0 the count doubles per
    # diamond, delta[a_k] = 3 (n - k), delta[b_k] = (1 + delta[a_{k+1}]) / 2
    def a(k):
        return base + 3 * k

    diamond = {}
    for k in range(DIAMONDS):
        b, c = a(k) + 1, a(k) + 2
        src += [a(k), a(k), b, c]
        dst += [b, c, a(k + 1), a(k + 1)]
        half = 0.5 * (1.0 + 3.0 * (DIAMONDS - k - 1))
        diamond[a(k)] = (3.0 * (DIAMONDS - k), 2.0 ** k, 2 * k)
        diamond[b] = diamond[c] = (half, 2.0 ** k, 2 * k + 1)
    diamond[a(DIAMONDS)] = (0.0, 2.0 ** DIAMONDS, 2 * DIAMONDS)
    cases.append(("diamonds", a(0), diamond))
    base = a(DIAMONDS) + 1

    # grid from the corner: sigma = C(i + j, i); delta by the recurrence over
    # the two deeper neighbours, in exact integer path counts
    def cell(i, j):
        return base + i * GRID + j

    sig = [[comb(i + j, i) for j in range(GRID)] for i in range(GRID)]
    dl = [[0.0] * GRID for _ in range(GRID)]
    for i in reversed(range(GRID)):
        for j in reversed(range(GRID)):
            for ni, nj in ((i + 1, j), (i, j + 1)):
                if ni < GRID and nj < GRID:
                    dl[i][j] += sig[i][j] / sig[ni][nj] * (1.0 + dl[ni][nj])
    grid = {}
    for i in range(GRID):
        for j in range(GRID):
            if i + 1 < GRID:
                src.append(cell(i, j))
                dst.append(cell(i + 1, j))
            if j + 1 < GRID:
                src.append(cell(i, j))
                dst.append(cell(i, j + 1))
            grid[cell(i, j)] = (dl[i][j], float(sig[i][j]), i + j)
    assert sig[GRID - 1][GRID - 1] == 8233430727600
    cases.append(("grid", cell(0, 0), grid))
    base += GRID * GRID

    path = {}
    for i in range(PATH):
        if i + 1 < PATH:
            src.append(base + i)
            dst.append(base + i + 1)
        path[base + i] = (float(PATH - 1 - i), 1.0, i)
    cases.append(("path", base, path))
    base += PATH

    cases.append(("isolated source", base + 3, {base + 3: (0.0, 1.0, 0)}))
    base += ISOLATED

    src += [base] * 3
    dst += [base + 1] * 3
    cases.append(("triple edge", base,
                  {base: (1.0, 1.0, 0), base + 1: (0.0, 3.0, 1)}))
    base += 2
    return (np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64),
            base, cases)


def check_closed_forms(eng, g, num_v, cases):
    """One bc call per case; returns the levels of each call."""
    rounds = []
    for name, source, known in cases:
        delta = np.zeros(num_v)
        sigma = np.zeros(num_v)
        depth = np.full(num_v, INT64_MAX, dtype=np.int64)
        for v, (dl, sg, dp) in known.items():
            delta[v], sigma[v], depth[v] = dl, sg, dp
        r = eng.bc(g, source)
        assert_result(r, (delta, sigma, depth), name)
        assert r["rounds"] == max(dp for _, _, dp in known.values()) + 1
        rounds.append(r["rounds"])
    return rounds


def test_closed_form_shapes(eng):
    src, dst, num_v, cases = shapes_graph()
    g = eng.load_edges(src, dst, directed=False, num_vertices=num_v)
    rounds = check_closed_forms(eng, g, num_v, cases)
    assert max(rounds) == 2 * DIAMONDS + 1


# --- 3. directed: the stored out-adjacency rule ----------------------------

def test_directed_out_adjacency(eng):
    rng = np.random.default_rng(93)
    src = rng.integers(0, 300, size=2000, dtype=np.int64)
    dst = rng.integers(0, 300, size=2000, dtype=np.int64)
    expect = oracle(300, src, dst, 2, directed=True)
    assert (expect[2] != INT64_MAX).sum() >= 290
    assert (expect[0] != 0).sum() >= 100
    g = eng.load_edges(src, dst, directed=True, num_vertices=300)
    assert_result(eng.bc(g, 2), expect, "directed")


# --- 4. arbitrary oids (hashmap idxer, padded owned range) -----------------

def test_arbitrary_oids(eng):
    rng = np.random.default_rng(95)
    si = rng.integers(0, 500, size=4000, dtype=np.int64)
    di = rng.integers(0, 500, size=4000, dtype=np.int64)
    oids = np.random.default_rng(96).choice(
        10**12, size=500, replace=False).astype(np.int64)
    g = eng.load_edges(oids[si], oids[di], directed=False, vertex_oids=oids,
                       idxer="hashmap")
    expect = oracle(500, si, di, 7, directed=False)
    r = eng.bc(g, int(oids[7]))  # the source is an oid
    assert set(r["oids"].tolist()) == set(oids.tolist())
    assert len(r["oids"]) == 500  # no padding rows
    pos = {int(o): i for i, o in enumerate(r["oids"].tolist())}
    take = np.array([pos[int(o)] for o in oids])
    assert_bc(np.asarray(r["values"])[take], np.asarray(r["path_num"])[take],
              np.asarray(r["depth"])[take], expect, "oids")


# --- 5. device-only graph ---------------------------------------------------

META_KEYS = ("rounds", "seconds", "traversed_edges", "bytes_p2p",
             "bytes_coll")


def brandes_identities(values, path_num, depth, source):
    """On symmetric storage the source's dependency counts the vertices it
    reaches, and the others' dependencies sum to the inner vertices of all
    shortest paths: sum over reached t of depth[t] - 1."""
    reach = depth != INT64_MAX
    reached = int(reach.sum())
    others = reach.copy()
    others[source] = False
    print("reached %d, max depth %d, delta[source] %.12g" %
          (reached, int(depth[reach].max()), values[source]))
    assert depth[source] == 0 and path_num[source] == 1
    assert np.isclose(values[source], reached - 1, rtol=1e-9, atol=1e-9)
    inner = float((depth[others] - 1).sum())
    assert np.isclose(values[others].sum(), inner, rtol=1e-9, atol=0.0)
    assert not values[~reach].any() and not path_num[~reach].any()
    return reached


def test_device_only_graph(eng):
    g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=5)
    r = eng.bc(g, 0)  # raised "needs a host fragment" before the GPU path
    assert np.array_equal(np.sort(r["oids"]), np.arange(20000))
    for key in META_KEYS:
        assert key in r, key
    depth = by_oid(r, "depth")
    assert np.array_equal(depth, by_oid(eng.bfs(g, 0)))
    reached = brandes_identities(by_oid(r), by_oid(r, "path_num"), depth, 0)
    assert reached > 2000  # the comparison is not about a handful of rows
    assert r["rounds"] == int(depth[depth != INT64_MAX].max()) + 1
    r = eng.bc(g, 0, values=False)
    for key in ("oids", "values", "path_num", "depth"):
        assert key not in r, key
    for key in META_KEYS:
        assert key in r, key


# --- 6. GPU equals host on RMAT --------------------------------------------

def test_gpu_equals_host_rmat(eng):
    # rmat_edges sizes are powers of two: draw 2^15 x 5 = 163,840 arcs,
    # fold the ids into 20,000 vertices and keep the first 160,000
    # (the synthetic graph itself is held to the oracles in
    # tests/test_gpu_synthetic_oracle.py, which models the generator's edges)
    src, dst, _, _ = grapehip.rmat_edges(15, edge_factor=5, seed=97)
    src, dst = src[:160000] % 20000, dst[:160000] % 20000
    source = int(src[0])
    cpu = grapehip.Engine(rank=0, world=1, master_port=29732)
    gc = cpu.load_edges(src, dst, directed=False, num_vertices=20000)
    gg = eng.load_edges(src, dst, directed=False, num_vertices=20000)
    c, g = cpu.bc(gc, source), eng.bc(gg, source)
    assert "traversed_edges" in g  # the GPU engine took the device path
    expect = (by_oid(c), by_oid(c, "path_num"), by_oid(c, "depth"))
    assert (expect[2] != INT64_MAX).sum() > 2000
    assert_result(g, expect, "rmat")


# --- 7. state hygiene -------------------------------------------------------

def test_state_hygiene(eng):
    rng = np.random.default_rng(98)
    nv = 3000
    src = rng.integers(0, nv, size=20000, dtype=np.int64)
    dst = rng.integers(0, nv, size=20000, dtype=np.int64)
    w = rng.integers(1, 100, size=20000).astype(np.float64)
    a, b = int(src[0]), int(src[1])
    assert a != b
    fresh = grapehip.Engine(rank=0, world=1, master_port=29733, gpu=True)
    gf = fresh.load_edges(src, dst, weights=w, directed=False,
                          num_vertices=nv)
    bfs0, sssp0 = by_oid(fresh.bfs(gf, b)), by_oid(fresh.sssp(gf, b))
    g = eng.load_edges(src, dst, weights=w, directed=False, num_vertices=nv)
    first = eng.bc(g, a)
    bfs1, sssp1 = by_oid(eng.bfs(g, b)), by_oid(eng.sssp(g, b))
    other = eng.bc(g, b)
    last = eng.bc(g, a)
    assert np.array_equal(bfs1, bfs0)
    assert np.array_equal(sssp1, sssp0)
    assert_result(first, oracle(nv, src, dst, a, directed=False), "first")
    assert_result(other, oracle(nv, src, dst, b, directed=False), "other")
    assert_result(last, (by_oid(first), by_oid(first, "path_num"),
                         by_oid(first, "depth")), "last")


# --- 8. multi-rank over the TCP-staged data plane ---------------------------

MULTI_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
import grapehip
eng = grapehip.engine_from_env(gpu=True)
g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7)
r = eng.bc(g, 0)
out = {k: r[k].tolist() for k in ("oids", "values", "path_num", "depth")}
out["bytes_p2p"] = int(r["bytes_p2p"])
out["rounds"] = int(r["rounds"])
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
    parts = [json.load(open(outdir / ("rank%d.json" % rank)))
             for rank in range(world)]
    oids = np.concatenate([np.array(d["oids"], dtype=np.int64)
                           for d in parts])
    assert np.array_equal(np.sort(oids), np.arange(20000))
    order = np.argsort(oids)
    merged = {}
    for key, dtype in (("values", np.float64), ("path_num", np.float64),
                       ("depth", np.int64)):
        merged[key] = np.concatenate(
            [np.array(d[key], dtype=dtype) for d in parts])[order]
    assert len({d["rounds"] for d in parts}) == 1  # ranks move in lockstep
    return merged, sum(d["bytes_p2p"] for d in parts)


def test_multirank_matches_single(tmp_path, free_port):
    single, sent = run_world(1, tmp_path / "w1", free_port)
    assert sent == 0
    expect = (single["values"], single["path_num"], single["depth"])
    assert brandes_identities(*expect, 0) > 2000
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        got, sent = run_world(world, tmp_path / ("w%d" % world), pick_port())
        assert sent > 0, world  # path counts and coefficients crossed
        assert_bc(got["values"], got["path_num"], got["depth"], expect,
                  "world %d" % world)


# --- 9. schedulers ----------------------------------------------------------

LB_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import grapehip
from test_gpu_bc import check_closed_forms, shapes_graph
src, dst, num_v, cases = shapes_graph()
eng = grapehip.Engine(rank=0, world=1, gpu=True)
g = eng.load_edges(src, dst, directed=False, num_vertices=num_v)
before = eng._debug_expand_counts()
rounds = check_closed_forms(eng, g, num_v, cases)
after = eng._debug_expand_counts()
# a forward expansion per level, a backward one per level but the source's
want = sum(2 * r - 1 for r in rounds)
lb = os.environ["GRAPEHIP_LB"]
for k in after:
    assert after[k] - before[k] == (want if k == lb else 0), (k, after, want)
print("RESULT ok %d" % want)
'''


def test_schedulers_agree():
    # GRAPEHIP_LB is read once per process: one process per scheduler
    procs = {}
    for lb in ("cm", "wm", "strict", "none"):
        env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_LB=lb)
        procs[lb] = subprocess.Popen([sys.executable, "-c", LB_WORKER],
                                     env=env, stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT)
    outs = {}
    try:
        for lb, p in procs.items():
            o, _ = p.communicate(timeout=120)
            outs[lb] = o.decode()
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    for lb, p in procs.items():
        assert p.returncode == 0, (lb, outs[lb])
        line = [x for x in outs[lb].splitlines() if x.startswith("RESULT ")]
        assert line, (lb, outs[lb])
        assert int(line[0].split()[2]) > 2 * DIAMONDS, lb


# --- 10. CLI ----------------------------------------------------------------

def test_cli_bc(tmp_path):
    rng = np.random.default_rng(99)
    nv = 300
    oids = np.arange(1, nv + 1, dtype=np.int64) * 3  # sparse, 1-based
    si = rng.integers(0, nv, 2000)
    di = rng.integers(0, nv, 2000)
    vfile, efile = tmp_path / "g.v", tmp_path / "g.e"
    np.savetxt(vfile, oids, fmt="%d")
    with open(efile, "w") as f:
        for a, b in zip(oids[si], oids[di]):
            f.write("%d %d\n" % (a, b))
    out = tmp_path / "gpu"
    source = int(si[0])
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application", "bc",
           "--bc_source", str(int(oids[source])), "--efile", str(efile),
           "--vfile", str(vfile), "--out_prefix", str(out), "--gpu"]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in open(out / "result_frag_0"):
        a, b = line.split()
        got[int(a)] = float(b)
    delta, _, depth = oracle(nv, si, di, source, directed=False)
    assert (depth != INT64_MAX).sum() >= 290 and delta.max() > 1
    assert set(got) == set(oids.tolist())
    vals = np.array([got[int(o)] for o in oids])
    assert np.allclose(vals, delta, rtol=1e-9, atol=1e-9)
