"""bench.py driver contract on one GPU: the result line, --steps, and
--dump-outputs (what the suite computes, indexed by a seeded vertex sample,
identical inputs from run to run). Sizes are tiny except that |V| sits just
above bench.DUMP_SAMPLE so the sampling branch is the one exercised."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import grapehip

REPO = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

NV, NE, SEED, PR_ITERS = 1_200_000, 4_800_000, 42, 3
NAMES = ("sample_oids", "bfs", "sssp", "pagerank")


def run_bench(outdir, *extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--nv", str(NV), "--ne", str(NE),
           "--seed", str(SEED), "--pr-iters", str(PR_ITERS),
           "--dump-outputs", str(outdir), *extra]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE")}
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {n: np.load(outdir / (n + ".npy"))
                                  for n in NAMES}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return run_bench(d / "a"), run_bench(d / "b", "--full")


def test_result_line(runs):
    for res, _ in runs:
        assert res["metric"] == "TEPS_bfs+sssp+pagerank_datagen-9_0-fb"
        assert res["unit"] == "TEPS" and res["higher_is_better"] is True
        assert res["dtype"] == "fp32/fp64"
        assert res["steps"] == 2 and res["warmup"] == 1
        assert res["ms_per_step"] > 0
        # value is edges traversed in the timed steps over their duration
        teps = (2 + PR_ITERS) * NE / (res["ms_per_step"] * 1e-3)
        assert res["value"] == pytest.approx(teps, rel=1e-9)


def test_dump_format(runs):
    _, out = runs[0]
    oids = out["sample_oids"]
    assert 0 < len(oids) < NV            # a sample, not every vertex
    assert (np.diff(oids) > 0).all() and oids[0] >= 0 and oids[-1] < NV
    total = 0
    for n in NAMES:
        assert out[n].dtype == np.float64 and out[n].shape == oids.shape
        total += out[n].nbytes
    assert total <= 64 << 20


def test_dump_repeatable(runs):
    (_, a), (_, b) = runs
    for n in ("sample_oids", "bfs", "sssp"):
        assert np.array_equal(a[n], b[n]), n
    # each run is within test_gpu_apps' PageRank tolerance (fp32
    # contributions, atomic order) of the exact ranks, so two runs are
    # within twice that of each other
    assert np.allclose(a["pagerank"], b["pagerank"], rtol=6e-5, atol=2e-12)


def test_dump_matches_engine(runs):
    _, out = runs[0]
    eng = grapehip.Engine(rank=0, world=1, master_port=29527, gpu=True)
    g = eng.load_synthetic(num_vertices=NV, num_edges=NE, seed=SEED,
                           directed=False, weighted=True)
    idx = out["sample_oids"].astype(np.int64)

    def by_oid(r):
        return np.asarray(r["values"])[np.argsort(r["oids"])][idx]

    assert np.array_equal(out["bfs"], by_oid(eng.bfs(g, 0)).astype(float))
    assert np.array_equal(out["sssp"], by_oid(eng.sssp(g, 0)))
    assert np.allclose(out["pagerank"],
                       by_oid(eng.pagerank(g, 0.85, PR_ITERS)),
                       rtol=6e-5, atol=2e-12)
