"""Host bc against GPU bc on the same RMAT edge lists (GPU box tool).

For each scale: rmat_edges(scale, edge_factor, seed), undirected, loaded on a
CPU engine and on a GPU engine; one host call (wall clock), one untimed and
--repeat timed GPU calls (the engine's barrier-bracketed seconds,
values=False), then one fetched GPU call compared with the host result.
Prints one JSON line per scale.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grapehip

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="18,20,21")
ap.add_argument("--edge-factor", type=int, default=4)
ap.add_argument("--seed", type=int, default=42)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
args = ap.parse_args()

cpu = grapehip.Engine(rank=0, world=1, master_port=29918,
                      n_threads=args.threads)
gpu = grapehip.Engine(rank=0, world=1, master_port=29919, gpu=True)


def by_oid(r, key):
    return np.asarray(r[key])[np.argsort(r["oids"])]


for scale in (int(x) for x in args.scales.split(",")):
    src, dst, _, _ = grapehip.rmat_edges(scale, edge_factor=args.edge_factor,
                                         seed=args.seed)
    nv = 1 << scale
    source = int(src[0])
    gc = cpu.load_edges(src, dst, directed=False, num_vertices=nv)
    t = time.time()
    c = cpu.bc(gc, source)
    host_s = time.time() - t
    del gc
    gg = gpu.load_edges(src, dst, directed=False, num_vertices=nv)
    gpu.bc(gg, source, values=False)
    ms = [round(gpu.bc(gg, source, values=False)["seconds"] * 1e3, 2)
          for _ in range(args.repeat)]
    g = gpu.bc(gg, source)
    depth = by_oid(c, "depth")
    reach = depth != np.iinfo(np.int64).max
    vc, vg = by_oid(c, "values"), by_oid(g, "values")
    print(json.dumps({
        "vertices": nv, "input_edges": len(src), "source": source,
        "host_s": round(host_s, 3), "host_engine_s": round(c["seconds"], 3),
        "gpu_ms": ms, "levels": g["rounds"], "reached": int(reach.sum()),
        "depth_equal": bool(np.array_equal(depth, by_oid(g, "depth"))),
        "path_num_equal": bool(np.array_equal(by_oid(c, "path_num"),
                                              by_oid(g, "path_num"))),
        "values_allclose_1e-9": bool(np.allclose(vg, vc, rtol=1e-9,
                                                 atol=1e-9)),
        "max_rel_err": float(np.max(np.abs(vg - vc) /
                                    np.maximum(np.abs(vc), 1.0))),
    }), flush=True)
    del gg
