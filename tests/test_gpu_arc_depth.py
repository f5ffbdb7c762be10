"""GRAPEHIP_ARC_DEPTH: the 64-arc windows whose gathers a wave of
pr_pull_seg_kernel keeps in flight.

Depth 1 is the unbatched loop; depths 2 and 4 must give the same bits:
PageRank ranks are np.array_equal to depth 1, with the segment path on and
with GRAPEHIP_PR_SEG=0, and depth 1 agrees with the oracle. The knobs are
read once per process, so every (mode, depth) is one fresh child process that
runs all graphs; children run one after another, each under its own timeout,
and nothing starts after one that died.

Modes (the segment knobs of test_gpu_pr_segments, HEAD=64 and IDS=128, in
all of them):
  seg256  items of 256 arcs: a wave quarter is one window
  seg     items of 4096 arcs: up to 16 windows per quarter (star_ring's hub)
  off     GRAPEHIP_PR_SEG=0, the row-tier pulls

The small pull and the frontier expansion are not batched (they were slower,
or gained less than the benchmark shows: profiles/r12_arc_depth.md), so no
graph here is aimed at them. The knob's parser is a static of the GPU engine
and is reached only through an Engine with a device, so there is no CPU-only
case for its fallback; the GPU case below checks it through
Engine._debug_arc_depth().
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
from test_gpu_pr_segments import (CASES as SEG_CASES, DAMPINGS, HEAD, IDS,
                                  _fan, _graph, _ring)

REPO = Path(__file__).resolve().parent.parent

RTOL, ATOL = 3e-5, 1e-12   # the project's PageRank tolerance
DEPTHS = (1, 2, 4)
MODES = {  # mode -> (GRAPEHIP_PR_SEG, GRAPEHIP_PR_SEG_ITEM)
    "seg256": ("1", "256"),
    "seg": ("1", None),
    "off": ("0", None),
}


def _slice(k, n=IDS):
    """The first n ids of slice k (1..8): ids HEAD + (k-1)*IDS onwards."""
    lo = HEAD + (k - 1) * IDS
    return np.arange(lo, lo + n)


def quarters():
    """Mid rows 5000..5013 with whole-slice spans, so that the slices' arc
    spaces (one item each at 4096 arcs per item, one batch) are
      slice 1: 2 x 128 + 30 = 286 arcs  -> quarters of 2 windows; at 256 arcs
               per item a last item of 30 arcs, shorter than a window
      slice 2: 3 x 128 + 100 = 484      -> 2 windows
      slice 3: 6 x 128 = 768            -> 3 windows, spans end on window ends
      slice 4: 8 x 128 = 1024           -> 4 windows
      slice 5: 10 x 128 = 1280          -> 5 windows
      slice 6: 40 arcs                  -> the whole arc space under 64 arcs,
               a quarter of 1 window
      slice 7: 7 x 96 = 672             -> 3 windows; the span at arcs 96..191
               runs from window 1 into window 2 (the group boundary at depth
               2), the one at 0..95 from window 0 into 1 (inside a group)
      slice 8: 14 x 96 = 1344           -> 6 windows; the span at arcs
               192..287 runs from window 3 into window 4 (the group boundary
               at depth 4)
    The ring stays below the rows."""
    nv = 6000
    parts = [_ring(4990)]
    for i in range(14):
        nb = []
        if i < 2: nb.append(_slice(1))
        if i == 2: nb.append(_slice(1, 30))
        if i < 3: nb.append(_slice(2))
        if i == 3: nb.append(_slice(2, 100))
        if i < 6: nb.append(_slice(3))
        if i < 8: nb.append(_slice(4))
        if i < 10: nb.append(_slice(5))
        if i == 0: nb.append(_slice(6, 40))
        if i < 7: nb.append(_slice(7, 96))
        nb.append(_slice(8, 96))
        parts.append(_fan(5000 + i, np.concatenate(nb)))
    return _graph(nv, parts)


# name -> builder; star_ring's hub span crosses every window and group
# boundary of its quarters at 4096 arcs per item
PR_CASES = dict(SEG_CASES, quarters=quarters)


WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_arc_depth import PR_CASES, DAMPINGS

eng = grapehip.Engine(rank=0, world=1, gpu=True)
out, arrays = {"depth": int(eng._debug_arc_depth())}, {}
if os.environ.get("ARC_DEPTH_KNOB_ONLY"):
    PR_CASES = {}

def by_oid(r):
    return np.asarray(r["values"])[np.argsort(np.asarray(r["oids"]))]

for name, build in PR_CASES.items():
    nv, src, dst = build()
    g = eng.load_edges(src, dst, directed=False, num_vertices=nv)
    eng._debug_pr_path(reset=True)
    # call 0 launches the kernels, call 1 captures the iteration, call 2
    # replays it, call 3 (another damping) captures again
    for i, d in enumerate((DAMPINGS[0],) * 3 + (DAMPINGS[1],)):
        arrays["pr/%s/%d" % (name, i)] = by_oid(eng.pagerank(g, d, 10))
    out[name] = dict(eng._debug_pr_path())
np.savez(os.environ["GRAPEHIP_OUT"], **arrays)
print("RESULT " + json.dumps(out))
'''


DEAD = []   # the first child that died or timed out, and why


def child(mode, depth, tmp, knob_only=False):
    """The results of one process at GRAPEHIP_ARC_DEPTH=depth; knob_only: it
    reports the depth in effect and runs no graph. After a child that died
    or timed out no other is started: every later call fails at once."""
    if DEAD:
        pytest.fail("no child is started after one that died: %r" % (DEAD[0],))
    return _child(mode, depth, tmp, knob_only)


@functools.lru_cache(maxsize=None)
def _child(mode, depth, tmp, knob_only):
    on, item = MODES[mode]
    out = Path(tmp) / ("%s_%s.npz" % (mode, depth))
    env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_OUT=str(out),
               GRAPEHIP_PR_SEG=on, GRAPEHIP_PR_SEG_HEAD=str(HEAD),
               GRAPEHIP_PR_SEG_IDS=str(IDS), GRAPEHIP_ARC_DEPTH=str(depth),
               ARC_DEPTH_KNOB_ONLY="1" if knob_only else "")
    for k in ("GRAPEHIP_PR_SEG_ITEM", "GRAPEHIP_PR_SEG_NT",
              "GRAPEHIP_PR_TILED"):
        env.pop(k, None)
    if item is not None:
        env["GRAPEHIP_PR_SEG_ITEM"] = item
    try:
        r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        DEAD.append((mode, depth, "timed out"))
        pytest.fail("child %s/%s timed out" % (mode, depth))
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or len(line) != 1:
        tail = r.stdout[-2000:] + r.stderr[-2000:]
        DEAD.append((mode, depth, "exit %d" % r.returncode, tail))
        pytest.fail("child %s/%s died: exit %d\n%s"
                    % (mode, depth, r.returncode, tail))
    return json.loads(line[0][len("RESULT "):]), np.load(out)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("arc_depth"))


@functools.lru_cache(maxsize=None)
def pr_oracle(name, damping):
    nv, src, dst = PR_CASES[name]()
    return pagerank_oracle(nv, src, dst, damping, 10, directed=False)


def test_graphs_hit_the_edges():
    """No GPU: the graphs are what their docstrings say."""
    nv, src, dst = quarters()
    want = {1: 286, 2: 484, 3: 768, 4: 1024, 5: 1280, 6: 40, 7: 672, 8: 1344}
    rows = src >= 5000
    for k, arcs in want.items():
        lo = HEAD + (k - 1) * IDS
        assert (rows & (dst >= lo) & (dst < lo + IDS)).sum() == arcs
    deg = np.bincount(np.concatenate([src, dst]), minlength=nv)
    assert deg[5000:5014].min() >= 64 and deg[:5000].max() < 64


@pytest.mark.gpu
def test_knob(tmp):
    """1, 2 and 4 are taken as given; anything else is the default, which a
    process with the knob empty reports."""
    for mode in MODES:
        for depth in DEPTHS:
            meta, _ = child(mode, depth, tmp)
            assert meta["depth"] == depth
    dflt, _ = child("seg", "", tmp, True)
    assert dflt["depth"] in DEPTHS
    meta, _ = child("seg", "3", tmp, True)
    assert meta["depth"] == dflt["depth"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PR_CASES))
@pytest.mark.parametrize("mode", list(MODES))
def test_pagerank(tmp, mode, name):
    _, one = child(mode, 1, tmp)
    seg_on = mode != "off" and name != "no_mid"   # no_mid has no mid row
    for depth in DEPTHS:
        meta, arr = child(mode, depth, tmp)
        assert meta[name] == ({"segments": 4, "rows": 0} if seg_on
                              else {"segments": 0, "rows": 4})
        for i, damping in enumerate((DAMPINGS[0],) * 3 + (DAMPINGS[1],)):
            got = arr["pr/%s/%d" % (name, i)]
            if depth == 1:
                expect = pr_oracle(name, damping)
                assert abs(got.sum() - 1.0) < 1e-5
                assert np.allclose(got, expect, rtol=RTOL, atol=ATOL), i
            else:
                assert np.array_equal(got, one["pr/%s/%d" % (name, i)]), \
                    (depth, i)
