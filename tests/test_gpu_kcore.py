"""GPU k-core / core decomposition (frontier peeling) on one MI355X: the HIP
path vs the NumPy oracles, closed-form shapes, the host engine, worlds 2 and
4 over the TCP-staged data plane, the four GRAPEHIP_LB schedulers and the
CLI. Results are integers, so every comparison is exact."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import grapehip
from oracles import coreness_oracle, kcore_oracle

REPO = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29721, gpu=True)


def by_oid(res):
    order = np.argsort(res["oids"])
    return np.asarray(res["values"])[order]


def multigraph(num_v=500, num_e=4000, loops=20, seed=91):
    """Endpoints drawn with replacement (duplicates occur) plus explicit
    self-loops."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, num_v, size=num_e, dtype=np.int64)
    dst = rng.integers(0, num_v, size=num_e, dtype=np.int64)
    lv = rng.choice(num_v, size=loops, replace=False).astype(np.int64)
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert len(pairs) < num_e  # the draw really produced duplicates
    return np.concatenate([src, lv]), np.concatenate([dst, lv])


# --- 1. oracle, random undirected multigraph -------------------------------

def test_oracle_random_undirected(eng):
    src, dst = multigraph()
    g = eng.load_edges(src, dst, directed=False, num_vertices=500)
    expect = coreness_oracle(500, src, dst)
    r = eng.core_decomposition(g)
    assert np.array_equal(np.sort(r["oids"]), np.arange(500))
    assert np.array_equal(by_oid(r), expect)
    max_core = int(expect.max())
    for k in (0, 1, 2, 3, 5, 8, max_core, max_core + 1):
        assert np.array_equal(by_oid(eng.kcore(g, k)),
                              kcore_oracle(500, src, dst, k)), k


# --- 2. closed-form shapes in one graph ------------------------------------

N_LEAVES = 5000
CLIQUE = 40
PATH = 10
ISOLATED = 7


def shapes_graph():
    """Star (hub row of 5000 arcs: crosses a 4096-arc boundary and many
    256-thread chunks), a disjoint 40-clique, a 10-vertex path, 7 isolated
    vertices and a pair joined by three parallel edges.
    Returns (src, dst, num_v, expected coreness)."""
    src, dst, core = [], [], []
    hub = 0
    src += [hub] * N_LEAVES
    dst += list(range(1, N_LEAVES + 1))
    core += [1] * (N_LEAVES + 1)
    base = N_LEAVES + 1
    for i in range(CLIQUE):
        for j in range(i + 1, CLIQUE):
            src.append(base + i)
            dst.append(base + j)
    core += [CLIQUE - 1] * CLIQUE
    base += CLIQUE
    for i in range(PATH - 1):
        src.append(base + i)
        dst.append(base + i + 1)
    core += [1] * PATH
    base += PATH
    core += [0] * ISOLATED
    base += ISOLATED
    src += [base] * 3
    dst += [base + 1] * 3
    core += [3, 3]
    base += 2
    return (np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64),
            base, np.array(core, dtype=np.int64))


def test_closed_form_shapes(eng):
    src, dst, num_v, expect = shapes_graph()
    g = eng.load_edges(src, dst, directed=False, num_vertices=num_v)
    r = eng.core_decomposition(g)
    assert np.array_equal(by_oid(r), expect)
    # levels 0, 1, 3 and 39 only: the jump from 3 to 39 visits nothing
    assert 4 <= r["rounds"] < CLIQUE
    in_clique = np.zeros(num_v, dtype=np.int64)
    in_clique[N_LEAVES + 1:N_LEAVES + 1 + CLIQUE] = 1
    keep2 = in_clique.copy()
    keep2[-2:] = 1  # the triple-edge pair
    assert np.array_equal(by_oid(eng.kcore(g, 2)), keep2)
    assert np.array_equal(by_oid(eng.kcore(g, CLIQUE - 1)), in_clique)
    assert not by_oid(eng.kcore(g, CLIQUE)).any()


# --- 3. directed: the stored out-adjacency rule ----------------------------

def test_directed_out_adjacency(eng):
    rng = np.random.default_rng(93)
    src = rng.integers(0, 300, size=2000, dtype=np.int64)
    dst = rng.integers(0, 300, size=2000, dtype=np.int64)
    g = eng.load_edges(src, dst, directed=True, num_vertices=300)
    expect = coreness_oracle(300, src, dst, directed=True)
    assert np.array_equal(by_oid(eng.core_decomposition(g)), expect)
    assert np.array_equal(by_oid(eng.kcore(g, 3)),
                          kcore_oracle(300, src, dst, 3, directed=True))


# --- 4. arbitrary oids (hashmap idxer, padded owned range) -----------------

def test_arbitrary_oids(eng):
    si, di = multigraph(seed=95)
    rng = np.random.default_rng(96)
    oids = rng.choice(10**12, size=500, replace=False).astype(np.int64)
    g = eng.load_edges(oids[si], oids[di], directed=False, vertex_oids=oids,
                       idxer="hashmap")
    expect = coreness_oracle(500, si, di)
    r = eng.core_decomposition(g)
    got = dict(zip(r["oids"].tolist(), r["values"].tolist()))
    assert set(got) == set(oids.tolist())
    assert [got[int(o)] for o in oids] == expect.tolist()
    for k in (2, int(expect.max())):
        r = eng.kcore(g, k)
        got = dict(zip(r["oids"].tolist(), r["values"].tolist()))
        assert set(got) == set(oids.tolist())
        assert ([got[int(o)] for o in oids] ==
                kcore_oracle(500, si, di, k).tolist()), k


# --- 5. device-only graph ---------------------------------------------------

@pytest.fixture(scope="module")
def synthetic(eng):
    return eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=5)


def test_device_only_graph_runs(eng, synthetic):
    r = eng.core_decomposition(synthetic)
    assert np.array_equal(np.sort(r["oids"]), np.arange(20000))
    core = by_oid(r)
    assert len(core) == 20000 and (core >= 0).all()
    top = int(core.max())
    assert top >= 2  # 160k edges on 20k vertices is not a forest
    for k in (1, 2, 3, top, top + 1):
        assert np.array_equal(by_oid(eng.kcore(synthetic, k)),
                              (core >= k).astype(np.int64)), k


def test_device_only_graph_result_dict(eng, synthetic):
    for r in (eng.core_decomposition(synthetic, values=False),
              eng.kcore(synthetic, 3, values=False)):
        assert "oids" not in r and "values" not in r
        for key in ("rounds", "seconds", "traversed_edges", "bytes_p2p",
                    "bytes_coll"):
            assert key in r, key
    r = eng.kcore(synthetic, k=3)
    assert len(r["values"]) == 20000 and "traversed_edges" in r


# --- 6. GPU equals host on RMAT --------------------------------------------

def test_gpu_equals_host_rmat(eng):
    # rmat_edges sizes are powers of two: draw 2^15 x 5 = 163,840 arcs,
    # fold the ids into 20,000 vertices and keep the first 160,000
    # (the synthetic graph itself is held to the oracles in
    # tests/test_gpu_synthetic_oracle.py, which models the generator's edges)
    src, dst, _, _ = grapehip.rmat_edges(15, edge_factor=5, seed=97)
    src, dst = src[:160000] % 20000, dst[:160000] % 20000
    cpu = grapehip.Engine(rank=0, world=1, master_port=29722)
    gc = cpu.load_edges(src, dst, directed=False, num_vertices=20000)
    gg = eng.load_edges(src, dst, directed=False, num_vertices=20000)
    c, g = cpu.core_decomposition(gc), eng.core_decomposition(gg)
    assert "traversed_edges" in g  # the GPU engine took the device path
    assert np.array_equal(by_oid(c), by_oid(g))
    assert np.array_equal(by_oid(cpu.kcore(gc, 4)), by_oid(eng.kcore(gg, 4)))


# --- 7. multi-rank over the TCP-staged data plane ---------------------------

MULTI_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
import grapehip
eng = grapehip.engine_from_env(gpu=True)
g = eng.load_synthetic(num_vertices=20000, num_edges=160000, seed=7)
out = {}
for name, r in (("core_decomposition", eng.core_decomposition(g)),
                ("kcore", eng.kcore(g, 3))):
    out[name] = {"oids": r["oids"].tolist(), "values": r["values"].tolist(),
                 "bytes_p2p": int(r["bytes_p2p"])}
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
    merged, sent = {}, 0
    for app in ("core_decomposition", "kcore"):
        oids, vals = [], []
        for rank in range(world):
            d = json.load(open(outdir / ("rank%d.json" % rank)))[app]
            oids.extend(d["oids"])
            vals.extend(d["values"])
            sent += d["bytes_p2p"]
        assert np.array_equal(np.sort(oids), np.arange(20000)), app
        merged[app] = np.array(vals)[np.argsort(oids)]
    return merged, sent


def test_multirank_matches_single(tmp_path, free_port):
    single, sent = run_world(1, tmp_path / "w1", free_port)
    assert sent == 0
    assert single["core_decomposition"].max() >= 3
    # a failing world raises here, so no further world is launched
    for world in (2, 4):
        got, sent = run_world(world, tmp_path / ("w%d" % world), pick_port())
        assert sent > 0, world  # decrement counts crossed the halo
        for app in ("core_decomposition", "kcore"):
            assert np.array_equal(got[app], single[app]), (world, app)


# --- 8. schedulers ----------------------------------------------------------

LB_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_kcore import shapes_graph
src, dst, num_v, _ = shapes_graph()
eng = grapehip.Engine(rank=0, world=1, gpu=True)
g = eng.load_edges(src, dst, directed=False, num_vertices=num_v)
r = eng.core_decomposition(g)
print("RESULT " + json.dumps(
    np.asarray(r["values"])[np.argsort(r["oids"])].tolist()))
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
    expect = shapes_graph()[3].tolist()
    for lb, p in procs.items():
        assert p.returncode == 0, (lb, outs[lb])
        line = [x for x in outs[lb].splitlines() if x.startswith("RESULT ")]
        assert line, (lb, outs[lb])
        assert json.loads(line[0][len("RESULT "):]) == expect, lb


# --- 9. CLI -----------------------------------------------------------------

def test_cli_core_decomposition(tmp_path):
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
    cmd = [sys.executable, "-m", "grapehip.run_app", "--application",
           "core_decomposition", "--efile", str(efile), "--vfile", str(vfile),
           "--out_prefix", str(out), "--gpu"]
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in open(out / "result_frag_0"):
        a, b = line.split()
        got[int(a)] = int(b)  # written as plain integers
    expect = coreness_oracle(nv, si, di)
    want = {int(oids[j]): int(expect[j]) for j in range(nv)}
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
