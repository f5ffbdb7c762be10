"""Host sampler against the device sampler on uploaded RMAT graphs, and the
device sampler alone on device-only graphs (GPU box tool).

--scales: for each scale, rmat_edges(scale, edge_factor, seed, weighted),
directed, loaded once into a GPU engine (host fragment + device graph). Per
strategy: one host call (device=False) of --host-walks walks, timed around the
call (the host path reports no seconds); one untimed and --repeat timed device
calls (device=True) of --walks walks, the engine's barrier-bracketed seconds.
The untimed call builds the index of the strategy; its build time and bytes
come from the debug hook. Steps per second = steps taken / seconds.

--synthetic NVxNE[,NVxNE...]: load_synthetic (weighted, undirected), device
calls only.

Starts are uniform over the vertex ids, the same list for both paths. Prints
one JSON line per graph. Under rocprofv3 use --repeat 1 --no-host and read the
sample_step_kernel dispatches in start order: one per hop.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grapehip

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="18,20,21")
ap.add_argument("--synthetic", default="")
ap.add_argument("--edge-factor", type=int, default=8)
ap.add_argument("--walks", type=int, default=1000000)
ap.add_argument("--host-walks", type=int, default=0,
                help="walks of the host call (0: as --walks)")
ap.add_argument("--hops", type=int, default=4)
ap.add_argument("--top-k", type=int, default=4)
ap.add_argument("--strategies", default="random,edge_weight,top_k")
ap.add_argument("--seed", type=int, default=42)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

gpu = grapehip.Engine(rank=0, world=1, master_port=29923,
                      n_threads=args.threads, gpu=True)
strategies = args.strategies.split(",")
host_walks = args.host_walks or args.walks


def device_runs(g, starts, out):
    for st in strategies:
        kw = dict(hops=args.hops, strategy=st, top_k=args.top_k, seed=7)
        before = gpu._debug_sample()
        r = gpu.sample(g, starts, device=True, **kw)
        hook = gpu._debug_sample()
        entry = {"steps": int(r["traversed_edges"]),
                 "rounds": int(r["rounds"])}
        if hook["cdf_builds"] > before["cdf_builds"]:
            entry["cdf_build_ms"] = round(hook["cdf_ms"], 3)
            entry["cdf_bytes"] = int(hook["cdf_bytes"])
        if hook["topk_builds"] > before["topk_builds"]:
            entry["topk_build_ms"] = round(hook["topk_ms"], 3)
            entry["topk_bytes"] = int(hook["topk_bytes"])
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            r = gpu.sample(g, starts, device=True, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            ms.append(round(r["seconds"] * 1e3, 3))
        entry["gpu_ms"] = ms
        entry["gpu_call_wall_ms_last"] = round(wall, 3)
        med = statistics.median(ms)
        entry["gpu_msteps_per_s"] = round(entry["steps"] / med / 1e3, 1)
        out.setdefault(st, {}).update(entry)


for scale in (int(x) for x in args.scales.split(",") if x):
    src, dst, w, nv = grapehip.rmat_edges(scale, edge_factor=args.edge_factor,
                                          seed=args.seed, weighted=True)
    g = gpu.load_edges(src, dst, weights=w, directed=True, num_vertices=nv)
    starts = np.random.default_rng(args.seed).integers(
        0, nv, size=args.walks, dtype=np.int64)
    out = {"graph": "rmat", "vertices": nv, "arcs": len(src),
           "walks": args.walks, "hops": args.hops, "k": args.top_k}
    device_runs(g, starts, out)
    if not args.no_host:
        out["host_walks"] = host_walks
        for st in strategies:
            t0 = time.perf_counter()
            r = gpu.sample(g, starts[:host_walks], hops=args.hops,
                           strategy=st, top_k=args.top_k, seed=7,
                           device=False)
            secs = time.perf_counter() - t0
            steps = int((r["paths"][:, 1:] >= 0).sum())
            e = out[st]
            e["host_s"] = round(secs, 3)
            e["host_steps"] = steps
            e["host_msteps_per_s"] = round(steps / secs / 1e6, 3)
            e["gpu_over_host"] = round(
                e["gpu_msteps_per_s"] / (steps / secs / 1e6), 1)
    print(json.dumps(out), flush=True)
    del g

for shape in (x for x in args.synthetic.split(",") if x):
    nv, ne = (int(x) for x in shape.split("x"))
    g = gpu.load_synthetic(num_vertices=nv, num_edges=ne, seed=7,
                           weighted=True)
    starts = np.random.default_rng(args.seed).integers(
        0, nv, size=args.walks, dtype=np.int64)
    out = {"graph": "load_synthetic", "vertices": nv, "input_edges": ne,
           "stored_arcs": int(g.num_edges), "walks": args.walks,
           "hops": args.hops, "k": args.top_k}
    device_runs(g, starts, out)
    print(json.dumps(out), flush=True)
    del g
