"""PageRank epilogue path: the small pull and the id-segment reduce apply a
row's sum themselves (next contribution, and the rank on the last iteration)
instead of storing it for pr_fused_apply_kernel, and the dangling sum of an
undirected graph is a scalar recurrence.

GRAPEHIP_PR_EPILOGUE is read once per process, so each setting is one fresh
child process that runs every graph; children run one after another, each
under its own timeout, and nothing starts after one that died. The fused path
under GRAPEHIP_PR_EPILOGUE=0 is the reference:

  * Given the same first dangling value both paths evaluate the same fp64
    expressions on the same row sums in the same order. They differ in that
    first value alone: n * (1/N) here, an atomic fp64 sum of n copies of 1/N
    there, with n the isolated vertices. Both round the same real number; the
    sum is off by at most (n - 1) * 2^-53 relative, and a rank's relative
    sensitivity to the dangling sum is at most 1. So rtol = n * 2^-52 per
    graph, computed from the graph, and np.array_equal when n = 0.
  * Against the host oracle: the project's PageRank tolerance.

The segment knobs of test_gpu_pr_segments (HEAD=64, IDS=128) put the segment
path on for graphs above 1088 ids; items of 256 arcs give the hub row of
`mixed` more than 64 partials, so the reduce's wave path runs next to its
lane path (the mid rows). A graph of at most 1088 ids has the segment path
off: the epilogue path then runs only if no row has 64 arcs or more
(`small_only`); with such a row (`segoff_mid`) the graph stays on the fused
path, as do a directed graph and a call with tol > 0.
"""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracles import pagerank_oracle
from test_gpu_pr_segments import DAMPINGS, HEAD, IDS, MID, _fan, _graph, _ring

REPO = Path(__file__).resolve().parent.parent

RTOL, ATOL = 3e-5, 1e-12   # the project's PageRank tolerance
ITERS = (1, 2, 3, 10)      # last iteration only, both parities, an odd count
# per (graph, iters), on one freshly loaded graph: call 0 records the
# iterations on the stream, call 1 captures them, call 2 replays, call 3
# (another damping) captures again, call 4 once more
CALLS = (DAMPINGS[0],) * 3 + (DAMPINGS[1], DAMPINGS[0])
SEG_TOP = HEAD + 8 * IDS   # the segment path is on above this many ids


def _mixed(extra):
    """Hub 0 with 17,000 arcs (hub tier; over 70 partials at 256 per item),
    a ring over ids 0..17996 (small rows of 2 and 3 arcs, some 70 chunks of
    256 rows), row 17500 with exactly 64 arcs (the first mid row), row 17600
    with 63 (small tier), ids 17997..17999 pendant (1 arc), then `extra`
    isolated ids."""
    nv = 18000
    return _graph(nv + extra, [
        _fan(0, np.arange(2, 17000)),           # + ring arcs to 1 and 17996
        _ring(nv - 3),
        _fan(17500, np.arange(100, 100 + 62 * 20, 20)),
        _fan(17600, np.arange(105, 105 + 61 * 20, 20)),
        _fan(17997, [5]), _fan(17998, [6]), _fan(17999, [7])])


def mixed():
    return _mixed(0)


def mixed_iso():
    return _mixed(777)


def small_only():
    """At most 1088 ids, so the segment path is off, and no row of 64 arcs:
    a ring of 700 (two whole chunks of 256 small rows and a part), row 800
    with 63 arcs, two pendants, 297 isolated ids."""
    return _graph(1000, [_ring(700), _fan(800, np.arange(0, 630, 10)),
                         _fan(801, [3]), _fan(802, [4])])


def segoff_mid():
    """The same with row 800 at 64 arcs: a mid row without the segment path
    goes through the row-tier pulls, which have no epilogue."""
    return _graph(1000, [_ring(700), _fan(800, np.arange(0, 640, 10))])


CASES = {"mixed": mixed, "mixed_iso": mixed_iso, "small_only": small_only}
FUSED_ONLY = {"segoff_mid": segoff_mid}


def n_isolated(name):
    nv, src, dst = dict(CASES, **FUSED_ONLY)[name]()
    return int((np.bincount(np.concatenate([src, dst]), minlength=nv)
                == 0).sum())


WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_pr_epilogue import CASES, FUSED_ONLY, ITERS, CALLS

eng = grapehip.Engine(rank=0, world=1, gpu=True)
out, arrays = {}, {}

def by_oid(r):
    return np.asarray(r["values"])[np.argsort(np.asarray(r["oids"]))]

def counts():
    c = dict(eng._debug_pr_epilogue(reset=True))
    c.update(eng._debug_pr_path(reset=True))
    return c

for name, build in CASES.items():
    nv, src, dst = build()
    for iters in ITERS:
        g = eng.load_edges(src, dst, directed=False, num_vertices=nv)
        counts()
        for i, d in enumerate(CALLS):
            arrays["%s/%d/%d" % (name, iters, i)] = by_oid(
                eng.pagerank(g, d, iters))
        out["%s/%d" % (name, iters)] = counts()

# these must stay on the fused path
nv, src, dst = FUSED_ONLY["segoff_mid"]()
g = eng.load_edges(src, dst, directed=False, num_vertices=nv)
for i in range(3):
    arrays["segoff_mid/%d" % i] = by_oid(eng.pagerank(g, 0.85, 10))
out["segoff_mid"] = counts()
nv, src, dst = CASES["mixed_iso"]()
g = eng.load_edges(src, dst, directed=True, num_vertices=nv,
                   build_in_csr=True)
for i in range(3):
    arrays["directed/%d" % i] = by_oid(eng.pagerank(g, 0.85, 10))
out["directed"] = counts()
g = eng.load_edges(src, dst, directed=False, num_vertices=nv)
for i in range(3):
    arrays["tol/%d" % i] = by_oid(eng.pagerank(g, 0.85, 10, tol=1e-9))
out["tol"] = counts()
np.savez(os.environ["GRAPEHIP_OUT"], **arrays)
print("RESULT " + json.dumps(out))
'''

DEAD = []   # the first child that died or timed out, and why


def child(knob, tmp):
    if DEAD:
        pytest.fail("no child is started after one that died: %r" % (DEAD[0],))
    return _child(knob, tmp)


@functools.lru_cache(maxsize=None)
def _child(knob, tmp):
    out = Path(tmp) / ("epi_%s.npz" % knob)
    env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_OUT=str(out),
               GRAPEHIP_PR_SEG="1", GRAPEHIP_PR_SEG_HEAD=str(HEAD),
               GRAPEHIP_PR_SEG_IDS=str(IDS), GRAPEHIP_PR_SEG_ITEM="256",
               GRAPEHIP_PR_EPILOGUE=knob)
    for k in ("GRAPEHIP_PR_SEG_NT", "GRAPEHIP_PR_TILED",
              "GRAPEHIP_ARC_DEPTH"):
        env.pop(k, None)
    if knob == "":
        del env["GRAPEHIP_PR_EPILOGUE"]
    try:
        r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        DEAD.append((knob, "timed out"))
        pytest.fail("child %r timed out" % knob)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or len(line) != 1:
        tail = r.stdout[-2000:] + r.stderr[-2000:]
        DEAD.append((knob, "exit %d" % r.returncode, tail))
        pytest.fail("child %r died: exit %d\n%s" % (knob, r.returncode, tail))
    return json.loads(line[0][len("RESULT "):]), np.load(out)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pr_epilogue"))


@functools.lru_cache(maxsize=None)
def oracle(name, damping, iters):
    nv, src, dst = CASES[name]()
    return pagerank_oracle(nv, src, dst, damping, iters, directed=False)


def test_graphs_hit_the_edges():
    """No GPU: the graphs are what their docstrings say."""
    def deg(case):
        nv, src, dst = case()
        return np.bincount(np.concatenate([src, dst]), minlength=nv)
    d = deg(mixed)
    assert d[0] > 16384 and d[17500] == MID
    nv, src, dst = mixed()
    tail = ((src == 0) & (dst >= SEG_TOP)).sum() + ((dst == 0) &
                                                    (src >= SEG_TOP)).sum()
    assert tail // 256 + 9 > 64        # the hub's partials at 256 per item
    assert d[17600] == MID - 1 and d[17997] == 1 and d.min() == 1
    assert set(np.unique(d[1:17997])) >= {2, 3}
    assert ((d > 0) & (d < MID)).sum() > 256
    assert ((d >= MID).sum(), mixed()[0] > SEG_TOP) == (2, True)
    assert n_isolated("mixed") == 0 and n_isolated("mixed_iso") == 777
    d = deg(small_only)
    assert d.max() == MID - 1 and small_only()[0] <= SEG_TOP
    assert (d > 0).sum() > 2 * 256 and (d > 0).sum() % 256 != 0
    assert n_isolated("small_only") > 0 and 1 in d and 2 in d
    d = deg(segoff_mid)
    assert d.max() == MID and segoff_mid()[0] <= SEG_TOP


@pytest.mark.gpu
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", list(CASES))
def test_ranks(tmp, name, iters):
    meta, arr = child("", tmp)
    meta0, arr0 = child("0", tmp)
    key = "%s/%d" % (name, iters)
    seg = name != "small_only"
    path = {"segments": len(CALLS), "rows": 0} if seg else \
        {"segments": 0, "rows": len(CALLS)}
    # every call took the epilogue path; all but the graph's first replayed
    # its iterations but the last from the captured pair
    assert meta[key] == dict(path, calls=len(CALLS),
                             replayed=(len(CALLS) - 1) * (iters - 1))
    assert meta0[key] == dict(path, calls=0, replayed=0)
    n = n_isolated(name)
    for i, damping in enumerate(CALLS):
        got, ref = arr["%s/%d" % (key, i)], arr0["%s/%d" % (key, i)]
        err = np.max(np.abs(got - ref) / np.abs(ref))
        print(key, "call", i, "isolated", n, "max rel diff to the fused path",
              err, "bound", n * 2.0 ** -52)
        if n == 0:
            assert np.array_equal(got, ref), (i, err)
        else:
            assert np.allclose(got, ref, rtol=n * 2.0 ** -52, atol=0.0), \
                (i, err)
        expect = oracle(name, damping, iters)
        assert abs(got.sum() - 1.0) < 1e-5
        assert np.allclose(got, expect, rtol=RTOL, atol=ATOL), (i, damping)
    # recorded, captured and replayed: the same bits; so after a re-capture
    for i in (1, 2, 4):
        assert np.array_equal(arr[key + "/0"], arr[key + "/%d" % i]), i


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["segoff_mid", "directed", "tol"])
def test_other_calls_stay_on_the_fused_path(tmp, what):
    """A mid row without the segment path, a directed graph and tol > 0."""
    meta, arr = child("", tmp)
    meta0, arr0 = child("0", tmp)
    assert meta[what]["calls"] == 0 and meta0[what]["calls"] == 0
    for i in range(3):
        assert np.array_equal(arr["%s/%d" % (what, i)],
                              arr0["%s/%d" % (what, i)]), i


@pytest.mark.gpu
def test_knob_values(tmp):
    """Unset takes the path and 0 does not (asserted per graph above); the
    two children saw the same graphs."""
    meta, _ = child("", tmp)
    meta0, _ = child("0", tmp)
    assert set(meta) == set(meta0)
    assert sum(m["calls"] for m in meta.values()) == \
        len(CASES) * len(ITERS) * len(CALLS)
