"""PageRank id-segment pull of the mid and hub rows.

The ids are cut into ten segments (a head, eight slices, a tail); a mid or
hub row's sorted adjacency is cut into one span per segment, the spans of a
segment form its arc space, and that is cut into items. With
GRAPEHIP_PR_SEG_HEAD=64 and GRAPEHIP_PR_SEG_IDS=128 the cuts are
0, 64, 192, ..., 1088, nv, so graphs of a few thousand vertices reach all
ten. The knobs are read once per process: every setting is one fresh child
process that runs all graphs; children run one after another, each under its
own timeout. A host-loaded graph with num_vertices given keeps its ids, so
the graphs below are laid out in id space.
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

REPO = Path(__file__).resolve().parent.parent

RTOL, ATOL = 3e-5, 1e-12   # the project's PageRank tolerance
HEAD, IDS = 64, 128
BOUNDS = [0] + [HEAD + k * IDS for k in range(9)]   # + nv
MID = 64                   # smallest degree of the mid tier
DAMPINGS = (0.85, 0.7)


def _ring(nv):
    a = np.arange(nv, dtype=np.int64)
    return a, (a + 1) % nv


def _fan(v, nbrs):
    nbrs = np.asarray(nbrs, dtype=np.int64)
    return np.full(len(nbrs), v, dtype=np.int64), nbrs


def _graph(nv, parts):
    src = np.concatenate([p[0] for p in parts])
    dst = np.concatenate([p[1] for p in parts])
    return nv, src, dst


def star_ring():
    """Hub 0 with 16,999 arcs (hub tier): a span in every segment, the tail
    span of 15,911 arcs crossing four items of 4096. The ring rows are small."""
    nv = 17000
    return _graph(nv, [_fan(0, np.arange(1, nv)), _ring(nv)])


def spans():
    """Row 5000: 70 arcs, all in slice 3 (ids 320..447). Row 5001: 40 arcs in
    slice 1 and 40 in the tail, nothing between. Row 5002: arcs in the head
    and the tail only. The ring stays below them, so they hold nothing else."""
    nv = 6000
    return _graph(nv, [_fan(5000, np.arange(330, 400)),
                       _fan(5001, np.r_[70:110, 3000:3040]),
                       _fan(5002, np.r_[0:50, 2000:2050]),
                       _ring(4990)])


def boundary():
    """Rows 5000, 5001 and 5002 each hold all of slice 2 (ids 192..319, 128
    arcs): every such span ends on the segment's last id, and with items of
    256 arcs the second one ends on an item boundary of the slice's arc
    space (the ring, over ids below 4990, puts no mid row in front of them). Row 5002
    goes on into slices 3 and 4."""
    nv = 6000
    return _graph(nv, [_fan(5000, np.arange(192, 320)),
                       _fan(5001, np.arange(192, 320)),
                       _fan(5002, np.arange(192, 500)),
                       _ring(4990)])


def threshold():
    """No ring: row 3000 has exactly 64 arcs (mid tier), row 3001 has 63 and
    stays on the small path; both spread over ids 0..1259."""
    nv = 4000
    return _graph(nv, [_fan(3000, np.arange(0, 1280, 20)),
                       _fan(3001, np.arange(5, 1265, 20))])


def no_mid():
    """A ring: no mid or hub row, the path switches itself off."""
    return _graph(3000, [_ring(3000)])


def iso_dup():
    """Row 2000 holds every id of 100..180 twice (162 arcs with duplicates,
    spans in the head's neighbour slices), row 2001 holds id 7 a hundred
    times; ids 2100..2999 and most below 2000 are isolated."""
    nv = 3000
    nb = np.repeat(np.arange(100, 181), 2)
    return _graph(nv, [_fan(2000, nb), _fan(2001, np.full(100, 7)),
                       _fan(2002, np.arange(1000, 1200))])


CASES = {"star_ring": star_ring, "spans": spans, "boundary": boundary,
         "threshold": threshold, "no_mid": no_mid, "iso_dup": iso_dup}
SEG_ARRAYS = ("bound", "rows", "span_first", "span_pref", "span_base",
              "span_row", "span_slot", "row_first", "off", "dst")

WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["GRAPEHIP_REPO"])
sys.path.insert(0, os.path.join(os.environ["GRAPEHIP_REPO"], "tests"))
import numpy as np
import grapehip
from test_gpu_pr_segments import CASES, DAMPINGS, SEG_ARRAYS

eng = grapehip.Engine(rank=0, world=1, gpu=True)
out, arrays = {}, {}
for name, build in CASES.items():
    nv, src, dst = build()
    g = eng.load_edges(src, dst, directed=False, num_vertices=nv)
    seg = eng._debug_pr_segments(g)
    out[name] = {"on": bool(seg["on"]), "item": int(seg["item"])}
    if seg["on"]:
        for k in SEG_ARRAYS:
            arrays[name + "/" + k] = np.asarray(seg[k])
    eng._debug_pr_path(reset=True)
    # call 0 launches the kernels, call 1 captures the iteration, call 2
    # replays it, call 3 (another damping) captures again
    for i, d in enumerate((DAMPINGS[0],) * 3 + (DAMPINGS[1],)):
        r = eng.pagerank(g, d, 10)
        if i == 0:
            assert np.array_equal(np.asarray(r["oids"]), np.arange(nv))
        arrays["%s/pr%d" % (name, i)] = np.asarray(r["values"])
    out[name]["path"] = dict(eng._debug_pr_path())
np.savez(os.environ["GRAPEHIP_OUT"], **arrays)
print("RESULT " + json.dumps(out))
'''

# setting -> (GRAPEHIP_PR_SEG, GRAPEHIP_PR_SEG_ITEM)
SETTINGS = {"seg": ("1", None), "seg256": ("1", "256"), "off": ("0", None)}


@functools.lru_cache(maxsize=None)
def child(setting, tmp):
    on, item = SETTINGS[setting]
    out = Path(tmp) / (setting + ".npz")
    env = dict(os.environ, GRAPEHIP_REPO=str(REPO), GRAPEHIP_OUT=str(out),
               GRAPEHIP_PR_SEG=on, GRAPEHIP_PR_SEG_HEAD=str(HEAD),
               GRAPEHIP_PR_SEG_IDS=str(IDS))
    for k in ("GRAPEHIP_PR_SEG_ITEM", "GRAPEHIP_PR_SEG_NT",
              "GRAPEHIP_PR_TILED"):
        env.pop(k, None)
    if item is not None:
        env["GRAPEHIP_PR_SEG_ITEM"] = item
    r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                       capture_output=True, text=True, timeout=120)
    # a child that died stops the test here: nothing else is launched
    assert r.returncode == 0, (setting, r.stdout[-2000:] + r.stderr[-2000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert len(line) == 1, (setting, r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(line[0][len("RESULT "):]), np.load(out)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pr_segments"))


@functools.lru_cache(maxsize=None)
def oracle(name, damping):
    nv, src, dst = CASES[name]()
    return pagerank_oracle(nv, src, dst, damping, 10, directed=False)


def test_graphs_hit_the_edges():
    """No GPU: the graphs are what their docstrings say."""
    def deg(case):
        nv, src, dst = case()
        return np.bincount(np.concatenate([src, dst]), minlength=nv)
    d = deg(star_ring)
    assert d[0] >= 16384 + 2 and d[1:].max() < MID
    d = deg(threshold)
    assert d[3000] == MID and d[3001] == MID - 1
    assert deg(no_mid).max() < MID
    d = deg(boundary)
    assert d[192:320].max() < MID and d[5000] == d[5001] == 128
    d = deg(iso_dup)
    assert d[2000] == 162 and d[2001] == 100 and (d == 0).sum() > 2000
    for case in CASES.values():
        assert case()[0] > BOUNDS[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("setting", ["seg", "seg256"])
def test_ranks(tmp, setting, name):
    meta, arr = child(setting, tmp)
    meta_off, arr_off = child("off", tmp)
    want_on = name != "no_mid"
    # the requested path ran, four calls each
    assert meta[name]["on"] == want_on
    assert meta[name]["path"] == ({"segments": 4, "rows": 0} if want_on
                                  else {"segments": 0, "rows": 4})
    assert not meta_off[name]["on"]
    assert meta_off[name]["path"] == {"segments": 0, "rows": 4}
    if want_on:
        assert meta[name]["item"] == (256 if setting == "seg256" else 4096)
    for i, damping in enumerate((DAMPINGS[0],) * 3 + (DAMPINGS[1],)):
        got = arr["%s/pr%d" % (name, i)]
        expect = oracle(name, damping)
        assert abs(got.sum() - 1.0) < 1e-5
        assert np.allclose(got, expect, rtol=RTOL, atol=ATOL), (i, damping)
        # fp64 sums of the same fp32 terms in another order
        ref = arr_off["%s/pr%d" % (name, i)]
        err = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
        print(setting, name, "call", i, "max rel diff to the row pulls", err)
        assert np.allclose(got, ref, rtol=1e-12, atol=0.0), (i, err)
    # launched, captured and replayed: the same bits
    assert np.array_equal(arr[name + "/pr0"], arr[name + "/pr1"])
    assert np.array_equal(arr[name + "/pr0"], arr[name + "/pr2"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "no_mid"])
@pytest.mark.parametrize("setting", ["seg", "seg256"])
def test_layout_invariants(tmp, setting, name):
    """Exactly once, from the layout alone: spans partition each row's
    adjacency, items partition each segment's arc space, every (span, item)
    piece has a partial of its own."""
    meta, arr = child(setting, tmp)
    a = {k: arr[name + "/" + k].astype(np.int64) for k in SEG_ARRAYS}
    item = meta[name]["item"]
    off, dst, rows = a["off"], a["dst"], a["rows"]
    nv = CASES[name]()[0]
    assert list(a["bound"]) == BOUNDS + [nv]
    deg = np.diff(off)
    assert np.array_equal(rows, np.nonzero(deg >= MID)[0])
    pref, base, srow = a["span_pref"], a["span_base"], a["span_row"]
    first = a["span_first"]
    nspan = len(base)
    assert len(pref) == nspan + 1 and first[0] == 0 and first[-1] == nspan
    assert np.all(np.diff(first) >= 0)
    length = np.diff(pref)
    assert pref[0] == 0 and np.all(length > 0)          # no empty span
    assert pref[-1] == deg[rows].sum()                  # every arc counted
    seg_of = np.searchsorted(first, np.arange(nspan), side="right") - 1
    # a span's arcs lie in its row and its segment
    for k in range(nspan):
        r = rows[srow[k]]
        assert off[r] <= base[k] and base[k] + length[k] <= off[r + 1]
        d = dst[base[k]:base[k] + length[k]]
        assert d.min() >= a["bound"][seg_of[k]]
        assert d.max() < a["bound"][seg_of[k] + 1]
    # spans of a segment are in row order; spans of a row tile its adjacency
    for s in range(10):
        assert np.all(np.diff(srow[first[s]:first[s + 1]]) > 0)
    order = np.lexsort((seg_of, srow))
    slot_expect = 0
    slots = []
    for j in range(len(rows)):
        mine = order[srow[order] == j]
        assert len(mine) and base[mine[0]] == off[rows[j]]
        assert np.array_equal(base[mine][1:], (base[mine] + length[mine])[:-1])
        assert base[mine[-1]] + length[mine[-1]] == off[rows[j] + 1]
        assert a["row_first"][j] == slot_expect
        for k in mine:                       # (segment, item) order
            lo = pref[k] - pref[first[seg_of[k]]]
            pieces = (lo + length[k] - 1) // item - lo // item + 1
            assert a["span_slot"][k] == slot_expect
            slots.append(np.arange(slot_expect, slot_expect + pieces))
            slot_expect += pieces
    assert a["row_first"][-1] == slot_expect
    # items tile every segment's arc space; the pieces are all distinct
    n_items = [-(-(pref[first[s + 1]] - pref[first[s]]) // item)
               for s in range(10)]
    assert sum(n_items) <= slot_expect <= sum(n_items) + nspan
    assert np.array_equal(np.concatenate(slots), np.arange(slot_expect))
    if name == "star_ring" and setting == "seg":
        assert length.max() >= 3 * 4096 and n_items[9] >= 4
    if name == "boundary" and setting == "seg256":
        k = first[2] + 1                     # row 5001's span in slice 2
        assert (pref[k + 1] - pref[first[2]]) % 256 == 0
        assert dst[base[k] + length[k] - 1] == BOUNDS[3] - 1
