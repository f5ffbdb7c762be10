"""Dump GPU LCC values so two builds can be compared (GPU box tool): the
tier graph of tests/test_gpu_lcc_tiers.py and a synthetic RMAT graph, each
undirected and directed, one .npy per run with the values ordered by oid."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import grapehip
from test_gpu_lcc_tiers import NV, build_edges

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--nv", type=int, default=2_000_000)
ap.add_argument("--ne", type=int, default=16_000_000)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)

eng = grapehip.Engine(rank=0, world=1, master_port=29917, gpu=True)
src, dst = build_edges()
for directed in (False, True):
    tag = "directed" if directed else "undirected"
    graphs = {
        "tiers": eng.load_edges(src, dst, directed=directed, num_vertices=NV,
                                build_in_csr=directed),
        "rmat": eng.load_synthetic(num_vertices=args.nv, num_edges=args.ne,
                                   seed=42, directed=directed,
                                   build_in_csr=directed),
    }
    for name, g in graphs.items():
        r = eng.lcc(g)
        vals = np.asarray(r["values"])[np.argsort(r["oids"])]
        np.save(os.path.join(args.out, "lcc_%s_%s.npy" % (name, tag)), vals)
        print(name, tag, len(vals), "nonzero", int(np.count_nonzero(vals)))
