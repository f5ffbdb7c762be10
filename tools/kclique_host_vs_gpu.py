"""Host kclique against GPU kclique, and GPU kclique k=3 against GPU lcc, on
the RMAT edge lists of tools/bc_host_vs_gpu.py (GPU box tool).

For each scale: rmat_edges(scale, edge_factor, seed), undirected, loaded on a
CPU engine and on a GPU engine. Per k: one host call (the engine's seconds;
skipped once a host call has taken longer than --host-budget seconds, and
then listed as null), one untimed and --repeat timed GPU calls (the engine's
barrier-bracketed seconds). lcc is timed the same way in the same process,
alternating with kclique k=3. Prints one JSON line per scale with the rows
per tier and the compiled kCliqueBlockMax.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grapehip

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="18,20,21")
ap.add_argument("--ks", default="3,4,5")
ap.add_argument("--edge-factor", type=int, default=4)
ap.add_argument("--seed", type=int, default=42)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--host-budget", type=float, default=60.0)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

cpu = grapehip.Engine(rank=0, world=1, master_port=29920,
                      n_threads=args.threads)
gpu = grapehip.Engine(rank=0, world=1, master_port=29921, gpu=True)
ks = [int(x) for x in args.ks.split(",")]

for scale in (int(x) for x in args.scales.split(",")):
    src, dst, _, _ = grapehip.rmat_edges(scale, edge_factor=args.edge_factor,
                                         seed=args.seed)
    nv = 1 << scale
    host = {}
    if not args.no_host:
        gc = cpu.load_edges(src, dst, directed=False, num_vertices=nv)
        over = False
        for k in ks:
            if over:
                host[k] = None
                continue
            r = cpu.kclique(gc, k)
            host[k] = (round(r["seconds"], 3), int(r["clique_count"]))
            over = r["seconds"] > args.host_budget
        del gc
    gg = gpu.load_edges(src, dst, directed=False, num_vertices=nv)
    out = {"vertices": nv, "input_edges": len(src),
           "block_max": int(gpu._debug_kclique()["block_max"])}
    for k in ks:
        c = int(gpu.kclique(gg, k)["clique_count"])
        hook = gpu._debug_kclique()
        ms = [round(gpu.kclique(gg, k)["seconds"] * 1e3, 2)
              for _ in range(args.repeat)]
        entry = {"count": c, "gpu_ms": ms,
                 "rows": [int(hook["rows_wave"]), int(hook["rows_block"]),
                          int(hook["rows_global"])]}
        if k in host:
            entry["host_s"] = host[k][0] if host[k] else None
            entry["equal"] = (host[k][1] == c) if host[k] else None
        out["k%d" % k] = entry
    gpu.lcc(gg, values=False)
    lcc_ms, k3_ms = [], []
    for _ in range(args.repeat):
        lcc_ms.append(round(gpu.lcc(gg, values=False)["seconds"] * 1e3, 2))
        k3_ms.append(round(gpu.kclique(gg, 3)["seconds"] * 1e3, 2))
    out["lcc_ms"] = lcc_ms
    out["k3_alternating_ms"] = k3_ms
    print(json.dumps(out), flush=True)
    del gg
