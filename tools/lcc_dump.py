"""Dump GPU LCC values and CDLP labels so two builds can be compared (GPU
box tool): the tier graphs of tests/test_gpu_lcc_tiers.py (lcc) and
tests/test_gpu_cdlp_tiers.py (cdlp, 10 iterations) and a synthetic RMAT graph
(both), each undirected and directed, one .npy per run with the values
ordered by oid."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import grapehip
import test_gpu_cdlp_tiers
import test_gpu_lcc_tiers

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--nv", type=int, default=2_000_000)
ap.add_argument("--ne", type=int, default=16_000_000)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)

eng = grapehip.Engine(rank=0, world=1, master_port=29917, gpu=True)
lsrc, ldst = test_gpu_lcc_tiers.build_edges()
csrc, cdst, cnv = test_gpu_cdlp_tiers.build_edges()


def dump(app, name, tag, r):
    vals = np.asarray(r["values"])[np.argsort(r["oids"])]
    np.save(os.path.join(args.out, "%s_%s_%s.npy" % (app, name, tag)), vals)
    print(app, name, tag, len(vals), "nonzero", int(np.count_nonzero(vals)))


for directed in (False, True):
    tag = "directed" if directed else "undirected"
    kw = dict(directed=directed, build_in_csr=directed)
    rmat = eng.load_synthetic(num_vertices=args.nv, num_edges=args.ne,
                              seed=42, **kw)
    dump("lcc", "tiers", tag,
         eng.lcc(eng.load_edges(lsrc, ldst, num_vertices=test_gpu_lcc_tiers.NV,
                                **kw)))
    dump("lcc", "rmat", tag, eng.lcc(rmat))
    dump("cdlp", "tiers", tag,
         eng.cdlp(eng.load_edges(csrc, cdst, num_vertices=cnv, **kw), 10))
    dump("cdlp", "rmat", tag, eng.cdlp(rmat, 10))
