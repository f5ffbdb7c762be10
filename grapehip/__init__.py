"""grapehip — an MI355X-native PIE graph-processing engine.

Brand-new implementation of the GRAPE PIE model (PEval/IncEval fixpoint over
edge-cut CSR fragments) with the capabilities of alibaba/libgrape-lite:
the six LDBC Graphalytics kernels (BFS, SSSP, PageRank, WCC, CDLP, LCC) on a
multithreaded CPU path and a hand-written HIP/CDNA4 GPU path, one process per
GPU, TCP control plane + RCCL-over-xGMI data plane.
"""
from __future__ import annotations

import os

from grapehip._core import Engine, Graph, WITH_HIP  # noqa: F401

from grapehip.generate import rmat_edges, uniform_edges  # noqa: F401
from grapehip.io import (read_ldbc_edges, read_ldbc_vertices,  # noqa: F401
                         load_string_edges, rebalance_partition)  # noqa: F401

__version__ = "0.1.0"


def fanout_parents(fanouts):
    """For each of the 1 + S columns of `Engine.sample_neighbors(...)["nodes"]`
    the column of its parent, -1 for column 0 (the seed).

    With L_0 = 1, L_h = L_{h-1} * f_h, level h starts at column
    c_h = 1 + L_1 + ... + L_{h-1} (c_0 = 0), and column c_h + j has its parent
    at column c_{h-1} + j // f_h.
    """
    import numpy as np

    parents = [np.array([-1], dtype=np.int64)]
    start, length = 0, 1  # first column and length of the level before
    for f in fanouts:
        f = int(f)
        if f < 1:
            raise ValueError("fanout = %d is below 1" % f)
        parents.append(start + np.arange(length * f, dtype=np.int64) // f)
        start, length = start + length, length * f
    return np.concatenate(parents)


def engine_from_env(n_threads: int = 0, gpu: bool = False,
                    port_offset: int = 17) -> Engine:
    """Create an Engine from torchrun-style env (RANK/WORLD_SIZE/MASTER_*).

    The engine's rendezvous port is MASTER_PORT + port_offset so it never
    collides with the launcher's own store.
    """
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    addr = os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(os.environ.get("MASTER_PORT", "29500")) + port_offset
    return Engine(rank=rank, world=world, master_addr=addr,
                  master_port=port, n_threads=n_threads, gpu=gpu)
