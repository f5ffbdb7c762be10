"""Stored test vectors: the p2p-31 LDBC-format graph (Gnutella peer-to-peer
network, SNAP) with the published per-vertex results for BFS / SSSP /
PageRank / WCC / CDLP / LCC, kept xz-compressed under tests/golden/p2p-31.

The loaders and the CLI read plain text files, so the set is unpacked once
per process into a temporary directory that is removed at exit.
"""
import atexit
import functools
import lzma
import shutil
import tempfile
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def p2p31_dir() -> Path:
    out = Path(tempfile.mkdtemp(prefix="grapehip_p2p31_"))
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    packed = sorted((GOLDEN / "p2p-31").glob("*.xz"))
    assert packed, "tests/golden/p2p-31 is empty"
    for src in packed:
        with lzma.open(src, "rb") as f, open(out / src.stem, "wb") as o:
            shutil.copyfileobj(f, o)
    return out
