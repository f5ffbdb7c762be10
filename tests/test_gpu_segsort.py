"""The shared segmented sort (adjacency sort of a built CSR, LCC's oriented
rows) through the `_debug_sort_rows` hook, against NumPy, exact."""
import numpy as np
import pytest

import grapehip

pytestmark = pytest.mark.gpu

# 0 and 1 are in no sort tier; 4096 | 4097 is the LDS | scratch boundary;
# 8192 | 8193 is a power-of-two pad boundary of the scratch path
ROW_LENGTHS = (0, 1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 20000)
LEAD, TAIL = 7, 5  # keys before the first row and after the last
TOP_KEY = 0xFFFFFFFE  # the largest key below the u32 padding value


@pytest.fixture(scope="module")
def eng():
    return grapehip.Engine(rank=0, world=1, master_port=29751, gpu=True)


@pytest.fixture(scope="module")
def csr():
    rng = np.random.default_rng(4096)
    lens = np.array(ROW_LENGTHS, dtype=np.uint64)
    rng.shuffle(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + LEAD
    n = int(off[-1]) + TAIL
    # a key range well under the key count: duplicates in every long row
    dst = rng.integers(0, 6000, size=n, dtype=np.uint32)
    # some spread over the whole u32 range, the top key several times
    wide = rng.choice(n, size=n // 8, replace=False)
    dst[wide] = rng.integers(0, TOP_KEY, size=len(wide), dtype=np.uint32)
    dst[rng.choice(n, size=64, replace=False)] = TOP_KEY
    for r in range(len(lens)):  # and the top key in every row of 2 or more
        if off[r + 1] - off[r] >= 2:
            dst[int(off[r])] = TOP_KEY
    assert dst.max() == TOP_KEY
    # positive weights from a few values: float order == bit order, and
    # equal (dst, w) pairs occur
    w = rng.integers(1, 40, size=n).astype(np.float32) * np.float32(0.25)
    for a in (off, dst, w):
        a.setflags(write=False)
    return off, dst, w


def rows(off):
    return [(int(off[r]), int(off[r + 1])) for r in range(len(off) - 1)]


def test_u32_rows_sorted(eng, csr):
    off, dst, _ = csr
    got = eng._debug_sort_rows(off, dst)
    assert got.dtype == np.uint32 and got.shape == dst.shape
    exp = dst.copy()
    for b, e in rows(off):
        exp[b:e] = np.sort(dst[b:e])
    for b, e in rows(off):
        assert np.array_equal(got[b:e], exp[b:e]), e - b
    # keys outside every row are untouched
    assert np.array_equal(got[:LEAD], dst[:LEAD])
    assert np.array_equal(got[-TAIL:], dst[-TAIL:])
    assert np.array_equal(got, exp)


def test_u64_rows_sorted_by_dst_then_weight_bits(eng, csr):
    off, dst, w = csr
    got_d, got_w = eng._debug_sort_rows(off, dst, w)
    assert got_d.dtype == np.uint32 and got_w.dtype == np.float32
    wbits = w.view(np.uint32)
    gbits = got_w.view(np.uint32)
    for b, e in rows(off):
        d, wb = got_d[b:e].astype(np.int64), gbits[b:e].astype(np.int64)
        assert np.all(np.diff(d) >= 0), e - b
        same = np.diff(d) == 0
        assert np.all(np.diff(wb)[same] >= 0), e - b
        # the packed-key order is unique, so this is multiset equality too
        order = np.lexsort((wbits[b:e], dst[b:e]))
        assert np.array_equal(got_d[b:e], dst[b:e][order]), e - b
        assert np.array_equal(gbits[b:e], wbits[b:e][order]), e - b
    for sl in (slice(None, LEAD), slice(-TAIL, None)):
        assert np.array_equal(got_d[sl], dst[sl])
        assert np.array_equal(gbits[sl], wbits[sl])


def test_degenerate_shapes(eng):
    none32 = np.zeros(0, dtype=np.uint32)
    nonef = np.zeros(0, dtype=np.float32)
    # rows but no arcs
    off = np.zeros(300, dtype=np.uint64)
    assert len(eng._debug_sort_rows(off, none32)) == 0
    d, w = eng._debug_sort_rows(off, none32, nonef)
    assert len(d) == 0 and len(w) == 0
    # no rows
    off = np.zeros(1, dtype=np.uint64)
    assert len(eng._debug_sort_rows(off, none32)) == 0
    d, w = eng._debug_sort_rows(off, none32, nonef)
    assert len(d) == 0 and len(w) == 0
