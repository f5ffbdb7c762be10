#!/usr/bin/env python3
"""grapehip flagship benchmark — the BASELINE.json headline metric:
LDBC Graphalytics makespan + TEPS for BFS / SSSP / PageRank on a
datagen-9_0-fb-shaped graph (|V|=404,817,003, |E|=1,010,447,118; synthetic
RMAT stand-in with random [1,100) weights — no network, no datasets), on
1..8 MI355X GPUs, strong scaling (fixed graph partitioned across ranks).

One "step" = one full suite run: BFS + SSSP + PageRank(10 iters) on the
resident graph. value = aggregate traversed-edges/second over the timed
steps (TEPS, whole-job across all ranks). The graph build (generation +
CSR in HBM) is untimed setup, like LDBC's load phase.

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  # N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
  #        --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: build the graph, warm
up, time the K steps, print one JSON result line.

  --dump-outputs DIR  after the timed steps, write the per-vertex results of
                      the suite (BFS depth, SSSP distance, PageRank rank) as
                      DIR/<name>.npy (float64), indexed by a fixed seeded
                      sample of vertex ids (DIR/sample_oids.npy), so two
                      builds can be compared output for output.
  --full              reserved for measurements beyond the headline figure
                      (baselines, other sizes or precisions). The benchmark
                      has none today, so the flag changes nothing yet.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# datagen-9_0-fb shape (LDBC Graphalytics XL dataset)
DATAGEN_9_0_FB_V = 404_817_003
DATAGEN_9_0_FB_E = 1_010_447_118

# Reference baseline for the same metric: aggregate TEPS of the suite at
# its published datagen-9_0-fb times (BFS 0.07s, SSSP 0.42s,
# PageRank 1.40s on 4x r6.8xlarge): (E + E + 10E) / 1.89s.
BASELINE_SUITE_TEPS = 12.0 * DATAGEN_9_0_FB_E / (0.07 + 0.42 + 1.40)


# --dump-outputs: vertices sampled per run (3 float64 arrays + the ids stay
# far below the 64 MB cap: 4 x 8 MB)
DUMP_SAMPLE = 1 << 20


def dump_outputs(outdir, eng, g, args, rank, world):
    """Write what the suite computes on the resident graph.

    The timed calls run with values=False: results stay on the device and
    the caller receives only counters. The same three calls are repeated
    here, untimed, with values=True, i.e. the arrays a caller of the suite
    receives. Rows come back in the engine's internal (hub-renumbered)
    order, so they are indexed by original vertex id: DIR/<name>.npy[i] is
    the value of vertex DIR/sample_oids.npy[i]. The sample depends only on
    --seed and --nv. With several ranks each writes the sampled vertices it
    owns, as <name>_rank<r>.npy.
    """
    import numpy as np

    if args.nv <= DUMP_SAMPLE:
        sample = np.arange(args.nv, dtype=np.int64)
    else:
        rng = np.random.default_rng(args.seed)
        sample = np.unique(rng.integers(0, args.nv, DUMP_SAMPLE))
    wanted = np.zeros(args.nv, dtype=bool)
    wanted[sample] = True

    os.makedirs(outdir, exist_ok=True)
    suffix = "" if world == 1 else "_rank%d" % rank
    rows = None
    for name, run in (
            ("bfs", lambda: eng.bfs(g, args.source)),
            ("sssp", lambda: eng.sssp(g, args.source)),
            ("pagerank", lambda: eng.pagerank(g, 0.85, args.pr_iters))):
        r = run()
        if rows is None:
            # same graph, same row order for all three results
            oids = r["oids"]
            rows = np.nonzero(wanted[oids])[0]
            mine = oids[rows]
            order = np.argsort(mine, kind="stable")
            rows, mine = rows[order], mine[order]
            np.save(os.path.join(outdir, "sample_oids%s.npy" % suffix),
                    mine.astype(np.float64))
            del oids
        np.save(os.path.join(outdir, name + suffix + ".npy"),
                np.asarray(r["values"])[rows].astype(np.float64))
        del r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--source", type=int, default=0)
    ap.add_argument("--pr-iters", type=int, default=10)
    ap.add_argument("--nv", type=int, default=DATAGEN_9_0_FB_V)
    ap.add_argument("--ne", type=int, default=DATAGEN_9_0_FB_E)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the suite's per-vertex results (seeded "
                         "vertex sample) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (none today)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    import grapehip

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))
    if world != args.gpus and "WORLD_SIZE" not in os.environ:
        world = args.gpus
    eng = grapehip.engine_from_env(gpu=True) if world > 1 or "RANK" in os.environ \
        else grapehip.Engine(rank=0, world=1, master_port=29517, gpu=True)

    t_build0 = time.time()
    g = eng.load_synthetic(num_vertices=args.nv, num_edges=args.ne,
                           seed=args.seed, directed=False, weighted=True)
    t_build = time.time() - t_build0

    def suite():
        # values=False: the timed region is the algorithm (the reference's
        # "run algorithm" LDBC phase); result output is a separate phase.
        r_bfs = eng.bfs(g, args.source, values=False)
        r_sssp = eng.sssp(g, args.source, values=False)
        r_pr = eng.pagerank(g, 0.85, args.pr_iters, values=False)
        # edge accounting matches the baseline computation: E per BFS/SSSP
        # run, E per PageRank iteration (input edges, not stored arcs)
        traversed = (2 + args.pr_iters) * g.input_edges
        return traversed, {"bfs_ms": r_bfs["seconds"] * 1e3,
                           "sssp_ms": r_sssp["seconds"] * 1e3,
                           "pr_ms": r_pr["seconds"] * 1e3,
                           "bfs_rounds": r_bfs["rounds"],
                           "sssp_rounds": r_sssp["rounds"]}

    for _ in range(args.warmup):
        suite()

    eng.barrier()
    eng.device_sync()
    t0 = time.time()
    traversed_total = 0
    last = {}
    for _ in range(args.steps):
        t, last = suite()
        traversed_total += t
    eng.device_sync()
    eng.barrier()
    t1 = time.time()

    elapsed = eng.allreduce_max(t1 - t0)
    teps = traversed_total / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, eng, g, args, rank, world)

    if rank == 0:
        out = {
            "metric": "TEPS_bfs+sssp+pagerank_datagen-9_0-fb",
            "value": teps,
            "unit": "TEPS",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": (teps / BASELINE_SUITE_TEPS
                            if (args.nv, args.ne) ==
                            (DATAGEN_9_0_FB_V, DATAGEN_9_0_FB_E) else None),
            "dtype": "fp32/fp64",
            "data": "synthetic",
            "config": {
                "model": "LDBC suite: BFS + SSSP + PageRank(x%d)" % args.pr_iters,
                "graph": "datagen-9_0-fb-shaped RMAT (synthetic)",
                "num_vertices": args.nv,
                "num_edges": args.ne,
                "stored_edges": g.num_edges,
                "weights": "uniform [1,100) fp32",
                "source": args.source,
                "parallelism": "graph partitioned over %d GPU(s), RCCL/xGMI halo" % world,
                "build_seconds": t_build,
                "per_app_last_step": last,
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
