"""load_synthetic on one MI355X against the NumPy model of its generator
(tests/synthetic_oracle.py).

Structure: the stored graph, read back with Engine._debug_csr and translated
to original ids, is the model's edge list, arc for arc and weight bit for
weight bit, for undirected weighted, directed with an in-CSR and unweighted
graphs, with the slice-balance scramble and the hub renumbering each on and
off (GRAPEHIP_SCRAMBLE, GRAPEHIP_RENUMBER: gen_synthetic reads both on every
call, so setting them before load_synthetic selects them in-process). Every
stored weight has to be the model's fused rounding; a kernel that used the
other form, or a mix, fails with the count of each.

Applications: every app of the engine runs on the synthetic graph and is
compared with the project's oracles fed the model's edges, at the tolerances
of the app's own test file, from the hub (vertex 0, the benchmark's source),
a vertex that is isolated in the model and an ordinary vertex, with the
renumbering on (results come back through the oid list of a permuted graph)
and off.

What each shape is for is asserted on the model's edges before the GPU is
touched."""
from functools import lru_cache

import numpy as np
import pytest

import grapehip
from oracles import (bfs_oracle, cdlp_oracle_fast, coreness_oracle_fast,
                     kclique_oracle, kcore_oracle, lcc_oracle,
                     pagerank_oracle, sssp_oracle_f32, wcc_oracle, INT64_MAX)
from synthetic_oracle import raw_stream, scramble_ids, synthetic_edges
from test_gpu_bc import assert_result as assert_bc_result
from test_gpu_bc import oracle as bc_expect
from test_sampler_draw_oracle import draw, pick_slot, walk_oracle

pytestmark = pytest.mark.gpu

SCRAMBLE, RENUMBER = "GRAPEHIP_SCRAMBLE", "GRAPEHIP_RENUMBER"
RENUM_CAP = 4095  # the last bucket of the renumber's counting sort
DEFAULT_ABC = (0.57, 0.19, 0.19)


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29751, gpu=True)


# name: nv, ne, seed, abc and what the model must show for the shape.
# hub: a stored (undirected) degree above the renumber cap, or below it;
# folds: raw ids >= nv exist; loops / isolated: at least one of each.
SHAPES = {
    "20000x160000": dict(nv=20000, ne=160000, seed=7, abc=DEFAULT_ABC,
                         hub=True, folds=True, loops=True, isolated=True),
    "6000x100000": dict(nv=6000, ne=100000, seed=5, abc=DEFAULT_ABC,
                        hub=True, folds=True, loops=True, isolated=True),
    "4096x40000": dict(nv=4096, ne=40000, seed=3, abc=DEFAULT_ABC,
                       hub=False, folds=False, loops=True, isolated=True),
    "5000x60000": dict(nv=5000, ne=60000, seed=11, abc=DEFAULT_ABC,
                       hub=False, folds=True, loops=True, isolated=True),
    "3x50": dict(nv=3, ne=50, seed=1, abc=DEFAULT_ABC,
                 hub=False, folds=True, loops=True, isolated=False),
    "2x50": dict(nv=2, ne=50, seed=1, abc=DEFAULT_ABC,
                 hub=False, folds=False, loops=True, isolated=False),
    "3000x30000abc": dict(nv=3000, ne=30000, seed=9, abc=(0.45, 0.25, 0.15),
                          hub=False, folds=True, loops=True, isolated=True),
}

# mode: directed, weighted, build_in_csr
MODES = {
    "undirected-weighted": (False, True, False),
    "directed-incsr": (True, True, True),
    "unweighted": (False, False, False),
}

ENVS = {
    "default": {},
    "norenumber": {RENUMBER: "0"},
    "noscramble": {SCRAMBLE: "0"},
    "plain": {SCRAMBLE: "0", RENUMBER: "0"},
}


@lru_cache(maxsize=None)
def model(shape, scramble=True, fused=True):
    """The model's (src, dst, w) of a shape; shared, never written to."""
    p = SHAPES[shape]
    out = synthetic_edges(p["nv"], p["ne"], p["seed"], True, *p["abc"],
                          scramble=scramble, fused=fused)
    for a in out:
        a.setflags(write=False)
    return out


def und_degree(nv, src, dst):
    """Stored degree of an undirected graph: a self-loop counts twice."""
    return np.bincount(np.concatenate([src, dst]), minlength=nv)


@lru_cache(maxsize=None)
def assert_model_conditions(shape):
    p = SHAPES[shape]
    nv, ne = p["nv"], p["ne"]
    for scramble in (True, False):
        src, dst, w = model(shape, scramble)
        deg = und_degree(nv, src, dst)
        if p["hub"]:
            assert deg.max() >= 4096 and deg[0] == deg.max(), shape
        else:
            assert deg.max() < RENUM_CAP, shape
        assert ((src == dst).sum() > 0) == p["loops"], shape
        assert ((deg == 0).sum() > 0) == p["isolated"], shape
    rs, rd, _ = raw_stream(nv, ne, p["seed"], *p["abc"])
    assert (((rs >= nv) | (rd >= nv)).sum() > 0) == p["folds"], shape
    assert p["folds"] == (nv & (nv - 1) != 0), shape
    if shape == "20000x160000":
        src, dst, _ = model(shape)
        deg = und_degree(nv, src, dst)
        assert (int(deg[0]), int((deg == 0).sum()),
                int((src == dst).sum())) == (5216, 5682, 112)
        _, _, split = model(shape, True, False)
        assert int((split != model(shape)[2]).sum()) == 1633
    if shape == "6000x100000":
        assert int(und_degree(nv, *model(shape)[:2]).max()) == 5663
    if shape == "4096x40000":
        assert int(und_degree(nv, *model(shape)[:2]).max()) == 3001
    return True


def load(eng, shape, directed, weighted, in_csr, env, mp):
    p = SHAPES[shape]
    mp.delenv(SCRAMBLE, raising=False)
    mp.delenv(RENUMBER, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    a, b, c = p["abc"]
    return eng.load_synthetic(num_vertices=p["nv"], num_edges=p["ne"],
                              seed=p["seed"], directed=directed,
                              weighted=weighted, build_in_csr=in_csr,
                              a=a, b=b, c=c)


def stored_arcs(c, side="out"):
    """(src, dst, w) of one stored CSR in original ids, in stored order."""
    pre = "" if side == "out" else "in_"
    off = c[pre + "off"].astype(np.int64)
    src = np.repeat(np.arange(len(off) - 1, dtype=np.int64) + c["v_begin"],
                    np.diff(off))
    dst = c[pre + "dst"].astype(np.int64)
    if c["old_of_new"] is not None:
        old = c["old_of_new"].astype(np.int64)
        src, dst = old[src], old[dst]
    return src, dst, c[pre + "w"]


def canon(src, dst, w):
    """The arc multiset in a canonical order: by (src, dst, weight bits)."""
    bits = (np.zeros(len(src), dtype=np.uint32) if w is None
            else np.ascontiguousarray(w, dtype=np.float32).view(np.uint32))
    order = np.lexsort((bits, dst, src))
    return src[order], dst[order], bits[order]


def assert_same_arcs(got, want, want_split, tag):
    """got and want as (src, dst, w). want_split: want with the weight's
    other rounding, for the message when the weights are not the fused
    form's."""
    gs, gd, gb = canon(*got)
    ws, wd, wb = canon(*want)
    assert len(gs) == len(ws), (tag, len(gs), len(ws))
    bad = np.flatnonzero((gs != ws) | (gd != wd))
    assert len(bad) == 0, (tag, "ids differ", len(bad), gs[bad[:5]],
                           gd[bad[:5]], ws[bad[:5]], wd[bad[:5]])
    if got[2] is None:
        assert want[2] is None, tag
        return
    n_fused = int((gb == wb).sum())
    n_split = int((gb == canon(*want_split)[2]).sum())
    print("%s: %d arcs, weights equal to the fused form %d, to the "
          "multiply-then-add form %d" % (tag, len(gs), n_fused, n_split))
    assert n_fused == len(gs), (tag, "weights", n_fused, n_split, len(gs))


def mirrored(src, dst, w):
    return (np.concatenate([src, dst]), np.concatenate([dst, src]),
            None if w is None else np.concatenate([w, w]))


def assert_rows_sorted(off, dst, w, tag):
    """Every row ascending by (dst, w) in stored ids."""
    off = off.astype(np.int64)
    if len(dst) < 2:
        return
    same_row = np.ones(len(dst) - 1, dtype=bool)
    inner = off[1:-1]
    same_row[inner[(inner > 0) & (inner < len(dst))] - 1] = False
    d0, d1 = dst[:-1].astype(np.int64), dst[1:].astype(np.int64)
    ok = d0 < d1
    if w is None:
        ok |= d0 == d1
    else:
        ok |= (d0 == d1) & (w[:-1] <= w[1:])
    assert (ok | ~same_row).all(), tag


# --- 1. structure -------------------------------------------------------------

@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_structure(eng, monkeypatch, shape, mode, env):
    assert assert_model_conditions(shape)
    p = SHAPES[shape]
    nv, ne = p["nv"], p["ne"]
    directed, weighted, in_csr = MODES[mode]
    scramble = ENVS[env].get(SCRAMBLE) != "0"
    renumber = ENVS[env].get(RENUMBER) != "0"
    tag = (shape, mode, env)
    src, dst, w = model(shape, scramble)
    _, _, w_split = model(shape, scramble, False)
    if not weighted:
        w = w_split = None
    # the two scramble settings describe one graph up to relabelling
    if not scramble:
        s_on, d_on, _ = model(shape, True)
        assert np.array_equal(scramble_ids(src, nv, p["seed"]), s_on)
        assert np.array_equal(scramble_ids(dst, nv, p["seed"]), d_on)

    g = load(eng, shape, directed, weighted, in_csr, ENVS[env], monkeypatch)
    c = eng._debug_csr(g)

    n_arcs = ne if directed else 2 * ne  # a self-loop is stored twice
    assert g.num_vertices == nv and g.input_edges == ne, tag
    assert g.num_edges == n_arcs, tag
    assert c["v_begin"] == 0, tag
    off = c["off"]
    assert len(off) == nv + 1 and off[0] == 0 and off[-1] == n_arcs, tag
    assert len(c["dst"]) == n_arcs and (np.diff(off.astype(np.int64)) >= 0).all()
    assert c["dst"].max() < nv, tag
    assert (c["w"] is None) == (not weighted), tag
    if weighted:
        assert c["w"].dtype == np.float32 and len(c["w"]) == n_arcs, tag
    has_in = directed and in_csr
    for key in ("in_off", "in_dst"):
        assert (c[key] is None) == (not has_in), (tag, key)
    assert (c["in_w"] is None) == (not (has_in and weighted)), tag

    # the renumbering: inverse bijections of [0, nv), hubs first
    for key in ("old_of_new", "new_of_old"):
        assert (c[key] is None) == (not renumber), (tag, key)
    if renumber:
        old, new = (c["old_of_new"].astype(np.int64),
                    c["new_of_old"].astype(np.int64))
        assert len(old) == len(new) == nv, tag
        assert np.array_equal(np.sort(old), np.arange(nv)), tag
        assert np.array_equal(np.sort(new), np.arange(nv)), tag
        assert np.array_equal(new[old], np.arange(nv)), tag
        assert np.array_equal(old[new], np.arange(nv)), tag
        capped = np.minimum(np.diff(off.astype(np.int64)), RENUM_CAP)
        assert (np.diff(capped) <= 0).all(), tag
        if p["hub"] and not directed:
            assert capped[0] == RENUM_CAP, tag  # the cap bucket is occupied

    assert_rows_sorted(off, c["dst"], c["w"], tag)

    # the arcs, in original ids
    want = (src, dst, w) if directed else mirrored(src, dst, w)
    want_split = ((src, dst, w_split) if directed
                  else mirrored(src, dst, w_split))
    out = stored_arcs(c)
    assert_same_arcs(out, want, want_split, tag + ("out",))
    if has_in:
        assert len(c["in_off"]) == nv + 1 and c["in_off"][-1] == ne, tag
        assert len(c["in_dst"]) == ne, tag
        assert_rows_sorted(c["in_off"], c["in_dst"], c["in_w"], tag)
        ins = stored_arcs(c, "in")
        assert_same_arcs(ins, (dst, src, w), (dst, src, w_split),
                         tag + ("in",))
        # and the in-CSR is the transpose of the out-CSR, weights included
        a, b = canon(*out), canon(ins[1], ins[0], ins[2])
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), tag

    if not renumber:
        # no relabelling in between: the stored arrays are the model's CSR
        ws, wd, wb = canon(*want)
        assert np.array_equal(
            off, np.concatenate([[0], np.cumsum(np.bincount(ws,
                                                            minlength=nv))]))
        assert np.array_equal(c["dst"], wd), tag
        if weighted:
            assert np.array_equal(c["w"].view(np.uint32), wb), tag


def test_debug_csr_copies_only(eng, monkeypatch):
    """Two reads return the same arrays, before and after an app ran, and an
    uploaded graph (never permuted) reads back too."""
    g = load(eng, "5000x60000", True, True, True, {}, monkeypatch)
    a = eng._debug_csr(g)
    before = eng.bfs(g, 0)["values"]
    b = eng._debug_csr(g)
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(eng.bfs(g, 0)["values"], before)
    src = np.array([0, 0, 2], dtype=np.int64)
    dst = np.array([1, 2, 1], dtype=np.int64)
    gu = eng.load_edges(src, dst, directed=True, num_vertices=4)
    c = eng._debug_csr(gu)
    assert c["off"][:5].tolist() == [0, 2, 2, 3, 3]
    assert c["dst"][:3].tolist() == [1, 2, 1]
    assert c["w"] is None and c["old_of_new"] is None
    assert c["new_of_old"] is None and c["in_off"] is None


# --- 2. applications ----------------------------------------------------------

# graph: shape, directed (weighted; directed with an in-CSR)
APP_GRAPHS = {"undirected": ("20000x160000", False),
              "directed": ("5000x60000", True)}
APP_ENVS = ("default", "norenumber")
_graphs = {}

app_cases = pytest.mark.parametrize("env", APP_ENVS)
both_graphs = pytest.mark.parametrize("graph", list(APP_GRAPHS))


def app_graph(eng, graph, env):
    """(g, nv, src, dst, w, directed); the device graph is loaded once per
    (graph, env) and shared."""
    shape, directed = APP_GRAPHS[graph]
    assert assert_model_conditions(shape)
    if (graph, env) not in _graphs:
        with pytest.MonkeyPatch.context() as mp:
            g = load(eng, shape, directed, True, directed, ENVS[env], mp)
        assert (eng._debug_csr(g)["old_of_new"] is None) == (
            env == "norenumber")
        _graphs[graph, env] = g
    src, dst, w = model(shape)
    return _graphs[graph, env], SHAPES[shape]["nv"], src, dst, w, directed


@lru_cache(maxsize=None)
def sources(graph):
    """The hub, a vertex isolated in the model and an ordinary vertex (the
    smallest id with 3..20 out-arcs and, directed, an in-arc)."""
    shape, directed = APP_GRAPHS[graph]
    nv = SHAPES[shape]["nv"]
    src, dst, _ = model(shape)
    deg = und_degree(nv, src, dst)
    out = deg if not directed else np.bincount(src, minlength=nv)
    into = deg if not directed else np.bincount(dst, minlength=nv)
    assert deg[0] == deg.max()
    isolated = int(np.flatnonzero(deg == 0)[nv // 8])  # not the first row
    ordinary = int(np.flatnonzero((out >= 3) & (out <= 20) & (into > 0))[0])
    assert ordinary > 0 and deg[isolated] == 0
    return 0, isolated, ordinary


def by_oid(r, nv, key="values"):
    """Values indexed by original id; the oid list must be a permutation."""
    oids = np.asarray(r["oids"])
    assert np.array_equal(np.sort(oids), np.arange(nv))
    return np.asarray(r[key])[np.argsort(oids)]


@lru_cache(maxsize=None)
def reference(graph, app, arg=None):
    """Oracle results on the model's edges, computed once and shared by the
    environments; read-only."""
    shape, directed = APP_GRAPHS[graph]
    nv = SHAPES[shape]["nv"]
    src, dst, w = model(shape)
    if app == "bfs":
        out = bfs_oracle(nv, src, dst, arg, directed=directed)
    elif app == "sssp":
        out = sssp_oracle_f32(nv, src, dst, w, arg, directed=directed)
    elif app == "pagerank":
        out = pagerank_oracle(nv, src, dst, 0.85, 10, directed=directed)
    elif app == "wcc":
        out = wcc_oracle(nv, src, dst)
    elif app == "cdlp":
        out = cdlp_oracle_fast(nv, src, dst, 5, directed=directed)
    elif app == "lcc":
        out = lcc_oracle(nv, src, dst, directed=directed)
    elif app == "coreness":
        out = coreness_oracle_fast(nv, src, dst, directed=directed)
    elif app == "kcore":
        out = kcore_oracle(nv, src, dst, arg, directed=directed)
    elif app == "bc":
        return bc_expect(nv, src, dst, arg, directed)
    elif app == "kclique":
        # the count does not depend on the names of the vertices, and the
        # oracle enumerates from the smaller id: hand it the graph renamed
        # by ascending degree, or the hub's row alone costs 5000^2 probes
        rank = np.empty(nv, dtype=np.int64)
        rank[np.argsort(und_degree(nv, src, dst), kind="stable")] = \
            np.arange(nv)
        return kclique_oracle(nv, rank[src], rank[dst], arg)
    else:
        raise KeyError(app)
    out.setflags(write=False)
    return out


@app_cases
@both_graphs
def test_bfs(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    hub, isolated, ordinary = sources(graph)
    for source in (hub, isolated, ordinary):
        expect = reference(graph, "bfs", source)
        if source == isolated:
            assert (expect != INT64_MAX).sum() == 1
        else:
            assert (expect != INT64_MAX).sum() > nv // 2
        got = by_oid(eng.bfs(g, source), nv)
        assert np.array_equal(got, expect), (graph, env, source)


@app_cases
@both_graphs
def test_sssp(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    for source in sources(graph):
        expect = reference(graph, "sssp", source)
        finite = expect < 1e300
        assert np.array_equal(
            finite, reference(graph, "bfs", source) != INT64_MAX)
        got = by_oid(eng.sssp(g, source), nv)
        assert np.array_equal(got >= 1e300, ~finite), (graph, env, source)
        # fp32 relaxation to convergence == fp32 Dijkstra, bit for bit
        assert np.array_equal(got[finite].astype(np.float32),
                              expect[finite].astype(np.float32)), (
            graph, env, source)


@app_cases
@both_graphs
def test_pagerank(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    got = by_oid(eng.pagerank(g, 0.85, 10), nv)
    expect = reference(graph, "pagerank")
    print("max rel err %.3e" % np.max(np.abs(got - expect) / expect))
    assert np.allclose(got, expect, rtol=3e-5, atol=1e-12), (graph, env)
    assert abs(got.sum() - 1.0) < 1e-5


@app_cases
@both_graphs
def test_wcc(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    expect = reference(graph, "wcc")  # the minimum original id
    assert len(np.unique(expect)) > 100  # isolated vertices label themselves
    assert np.array_equal(by_oid(eng.wcc(g), nv), expect), (graph, env)


@app_cases
@both_graphs
def test_cdlp(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    expect = reference(graph, "cdlp")  # labels are original ids
    assert 100 < len(np.unique(expect)) < nv
    assert np.array_equal(by_oid(eng.cdlp(g, 5), nv), expect), (graph, env)


@app_cases
@both_graphs
def test_lcc(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    expect = reference(graph, "lcc")
    assert (expect > 0).sum() > nv // 4
    assert np.allclose(by_oid(eng.lcc(g), nv), expect, rtol=1e-12), (
        graph, env)


@app_cases
@both_graphs
def test_core_decomposition_and_kcore(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    expect = reference(graph, "coreness")
    assert expect.max() > 20
    assert np.array_equal(by_oid(eng.core_decomposition(g), nv), expect), (
        graph, env)
    for k in (3, 20):
        want = reference(graph, "kcore", k)
        assert 0 < want.sum() < nv
        assert np.array_equal(by_oid(eng.kcore(g, k), nv), want), (
            graph, env, k)


@app_cases
@both_graphs
def test_bc(eng, graph, env):
    g, nv, *_ = app_graph(eng, graph, env)
    for source in sources(graph):
        assert_bc_result(eng.bc(g, source), reference(graph, "bc", source),
                         str((graph, env, source)))


@app_cases
@pytest.mark.parametrize("k", (3, 4))
def test_kclique(eng, env, k):
    g, *_ = app_graph(eng, "undirected", env)
    want = reference("undirected", "kclique", k)
    assert want > 100000
    before = eng._debug_kclique()["calls"]
    assert int(eng.kclique(g, k)["clique_count"]) == want, (env, k)
    assert eng._debug_kclique()["calls"] == before + 1


def walk_on_rows(off, adj, starts, hops, seed):
    """The uniform walk of test_sampler_draw_oracle on rows given in their
    stored order (off, adj in original ids, row v at off[v])."""
    nv = len(off) - 1
    starts = np.asarray(starts, dtype=np.int64)
    walk_ids = np.nonzero((starts >= 0) & (starts < nv))[0]
    paths = np.full((len(walk_ids), hops + 1), -1, dtype=np.int64)
    for row, walk in enumerate(walk_ids):
        v = int(starts[walk])
        paths[row, 0] = v
        for hop in range(hops):
            b, e = int(off[v]), int(off[v + 1])
            if e == b:
                break
            v = int(adj[b + pick_slot(draw(seed, int(walk), hop), None,
                                      e - b, "random", 0)])
            paths[row, hop + 1] = v
    return walk_ids.astype(np.int64), paths


@app_cases
@both_graphs
def test_sample_uniform(eng, graph, env):
    """A uniform walk takes slot index(r, deg) of the stored row, and the
    stored order of a renumbered graph is by new id: the oracle walks the
    rows of _debug_csr (which test_structure ties to the model) in original
    ids. Without the renumbering that order is the oracle's own."""
    g, nv, src, dst, w, directed = app_graph(eng, graph, env)
    hub, isolated, ordinary = sources(graph)
    starts = np.concatenate([np.arange(0, nv, nv // 250),
                             [hub, isolated, ordinary, nv + 5, -1, hub]])
    c = eng._debug_csr(g)
    s_old, d_old, _ = stored_arcs(c)
    order = np.argsort(s_old, kind="stable")  # rows by original id
    off = np.concatenate([[0], np.cumsum(np.bincount(s_old, minlength=nv))])
    want = walk_on_rows(off, d_old[order], starts, 4, 7)
    if env == "norenumber":
        direct = walk_oracle(nv, src, dst, None, starts, 4, "random", seed=7,
                             directed=directed)
        assert np.array_equal(direct[1], want[1])
    assert (want[1][:, -1] >= 0).sum() > 100  # most walks go the distance
    before = eng._debug_sample()["calls"]
    r = eng.sample(g, starts, hops=4, strategy="random", seed=7, device=True)
    assert eng._debug_sample()["calls"] == before + 1
    assert np.array_equal(r["walk_ids"], want[0]), (graph, env)
    bad = np.nonzero((r["paths"] != want[1]).any(axis=1))[0]
    assert len(bad) == 0, (graph, env, bad[:5], r["paths"][bad[:5]],
                           want[1][bad[:5]])
    assert r["traversed_edges"] == int((want[1][:, 1:] >= 0).sum())
