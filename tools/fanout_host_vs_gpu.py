"""Host fan-out sampler against the device one on uploaded RMAT graphs, and
the device one alone on device-only graphs (GPU box tool).

--workloads SEEDSxF1-F2[-...][,...]: e.g. 100000x10-10,10000x15-10-5.

--scales: for each scale, rmat_edges(scale, edge_factor, seed, weighted),
directed, loaded once into a GPU engine (host fragment + device graph). Per
workload and strategy: one untimed and --repeat timed device calls
(device=True), the engine's barrier-bracketed seconds; one host call
(device=False) of --host-seeds seeds, timed around the call (the host path
reports no seconds). Draws per second = samples drawn / seconds.

--synthetic NVxNE[,NVxNE...]: load_synthetic (weighted, undirected), device
calls only.

Seeds are uniform over the vertex ids, the same list for both paths. Prints
one JSON line per graph and workload. Under rocprofv3 use --repeat 1 --no-host
and read the fanout_level_kernel dispatches in start order: one per level.

--no-replace: every call with replace=False (fanout_level_norep_kernel);
edge_weight is dropped from the strategies, as the graphs here are weighted.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grapehip

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="18,20,21")
ap.add_argument("--synthetic", default="")
ap.add_argument("--edge-factor", type=int, default=8)
ap.add_argument("--workloads", default="100000x10-10,10000x15-10-5")
ap.add_argument("--host-seeds", type=int, default=0,
                help="seeds of the host call (0: as the workload)")
ap.add_argument("--top-k", type=int, default=4)
ap.add_argument("--strategies", default="random,edge_weight,top_k")
ap.add_argument("--seed", type=int, default=42)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-replace", action="store_true")
args = ap.parse_args()
replace = not args.no_replace

gpu = grapehip.Engine(rank=0, world=1, master_port=29924,
                      n_threads=args.threads, gpu=True)
strategies = [s for s in args.strategies.split(",")
              if replace or s != "edge_weight"]
workloads = []
for spec in args.workloads.split(","):
    n, fan = spec.split("x")
    workloads.append((int(n), [int(f) for f in fan.split("-")]))


def device_runs(g, seeds, fanouts, out):
    for st in strategies:
        kw = dict(strategy=st, top_k=args.top_k, seed=7, replace=replace)
        r = gpu.sample_neighbors(g, seeds, fanouts, device=True, **kw)
        offs = r["level_offsets"]
        entry = {"draws": int(r["traversed_edges"]),
                 "rounds": int(r["rounds"]),
                 "last_level_draws": int(
                     (r["nodes"][:, offs[-2]:] >= 0).sum()) if fanouts else 0}
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            r = gpu.sample_neighbors(g, seeds, fanouts, device=True, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            ms.append(round(r["seconds"] * 1e3, 3))
        entry["gpu_ms"] = ms
        entry["gpu_call_wall_ms_last"] = round(wall, 3)
        med = statistics.median(ms)
        entry["gpu_mdraws_per_s"] = round(entry["draws"] / med / 1e3, 1)
        out.setdefault(st, {}).update(entry)


def host_runs(g, seeds, fanouts, out):
    n_host = args.host_seeds or len(seeds)
    out["host_seeds"] = min(n_host, len(seeds))
    for st in strategies:
        t0 = time.perf_counter()
        r = gpu.sample_neighbors(g, seeds[:n_host], fanouts, strategy=st,
                                 top_k=args.top_k, seed=7, device=False,
                                 replace=replace)
        secs = time.perf_counter() - t0
        draws = int((r["nodes"][:, 1:] >= 0).sum())
        e = out[st]
        e["host_s"] = round(secs, 3)
        e["host_draws"] = draws
        e["host_mdraws_per_s"] = round(draws / secs / 1e6, 3)


for scale in (int(x) for x in args.scales.split(",") if x):
    src, dst, w, nv = grapehip.rmat_edges(scale, edge_factor=args.edge_factor,
                                          seed=args.seed, weighted=True)
    g = gpu.load_edges(src, dst, weights=w, directed=True, num_vertices=nv)
    for n, fanouts in workloads:
        seeds = np.random.default_rng(args.seed).integers(
            0, nv, size=n, dtype=np.int64)
        out = {"graph": "rmat", "vertices": nv, "arcs": len(src), "seeds": n,
               "fanouts": fanouts, "k": args.top_k, "replace": replace}
        device_runs(g, seeds, fanouts, out)
        if not args.no_host:
            host_runs(g, seeds, fanouts, out)
        print(json.dumps(out), flush=True)
    del g

for shape in (x for x in args.synthetic.split(",") if x):
    nv, ne = (int(x) for x in shape.split("x"))
    g = gpu.load_synthetic(num_vertices=nv, num_edges=ne, seed=7,
                           weighted=True)
    for n, fanouts in workloads:
        seeds = np.random.default_rng(args.seed).integers(
            0, nv, size=n, dtype=np.int64)
        out = {"graph": "load_synthetic", "vertices": nv, "input_edges": ne,
               "stored_arcs": int(g.num_edges), "seeds": n,
               "fanouts": fanouts, "k": args.top_k, "replace": replace}
        device_runs(g, seeds, fanouts, out)
        print(json.dumps(out), flush=True)
    del g
