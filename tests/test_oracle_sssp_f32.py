"""sssp_oracle_f32 against the model it stands for and against the fp64
oracle. The GPU engine relaxes arcs in an arbitrary order with possibly stale
source distances, lowers the target with an atomic min and re-queues every
vertex it lowers; run to its fixpoint, that must be bit-equal to Dijkstra in
fp32 arithmetic, because fp32 addition is monotone."""
import numpy as np
import pytest

from oracles import DBL_MAX, bfs_oracle, sssp_oracle, sssp_oracle_f32

F32_MAX = float(np.finfo(np.float32).max)


def graph(num_v, num_e, seed):
    """Random multigraph, weights in [1,10) with 5% exactly 0, 50 parallel
    pairs with the lighter arc second, 10 self-loops, a block of vertices
    without arcs."""
    rng = np.random.default_rng(seed)
    live = num_v - 20
    src = rng.integers(0, live, num_e).astype(np.int64)
    dst = rng.integers(0, live, num_e).astype(np.int64)
    w = (rng.random(num_e, dtype=np.float32) * 9 + 1).astype(np.float32)
    w[rng.random(num_e) < 0.05] = 0.0
    ps = rng.integers(0, live, 50).astype(np.int64)
    pd = rng.integers(0, live, 50).astype(np.int64)
    heavy = (rng.random(50, dtype=np.float32) * 4 + 5).astype(np.float32)
    light = (rng.random(50, dtype=np.float32) * 3 + 1).astype(np.float32)
    lv = rng.integers(0, live, 10).astype(np.int64)
    lw = (rng.random(10, dtype=np.float32) * 9 + 1).astype(np.float32)
    src = np.concatenate([src, np.stack([ps, ps], 1).ravel(), lv])
    dst = np.concatenate([dst, np.stack([pd, pd], 1).ravel(), lv])
    w = np.concatenate([w, np.stack([heavy, light], 1).ravel(), lw])
    return src, dst, w


def stale_fixpoint(num_v, src, dst, w, source, directed, seed):
    """The engine's model: each round relaxes a random subset of the arcs
    whose source is queued, all from one snapshot of dist (stale reads), in
    fp32; lowered targets are queued; a source leaves the queue only in a
    round that relaxed all its arcs, unless lowered again. Runs until the
    queue is empty."""
    rng = np.random.default_rng(seed)
    s = np.asarray(src, dtype=np.int64)
    d = np.asarray(dst, dtype=np.int64)
    ww = np.asarray(w, dtype=np.float32)
    if not directed:
        s, d, ww = (np.concatenate([s, d]), np.concatenate([d, s]),
                    np.concatenate([ww, ww]))
    dist = np.full(num_v, F32_MAX, dtype=np.float32)
    dist[source] = 0
    queued = np.zeros(num_v, bool)
    queued[source] = True
    rounds = 0
    while queued.any():
        rounds += 1
        assert rounds < 100000
        # 60% of the queued vertices relax all their arcs and leave the
        # queue; the others relax a random half of theirs and stay
        leave = queued & (rng.random(num_v) < 0.6)
        live = np.flatnonzero(queued[s])
        take = live[leave[s[live]] | (rng.random(len(live)) < 0.5)]
        snap = dist.copy()
        nd = snap[s[take]] + ww[take]
        assert nd.dtype == np.float32
        np.minimum.at(dist, d[take], nd)
        lowered = dist < snap
        queued = (queued & ~leave) | lowered
    out = dist.astype(np.float64)
    out[dist == np.float32(F32_MAX)] = DBL_MAX
    return out


CASES = [(500, 3000, True, 11), (500, 3000, False, 12),
         (3000, 20000, True, 13), (3000, 20000, False, 14)]


@pytest.mark.parametrize("num_v,num_e,directed,seed", CASES)
def test_f32_dijkstra_is_the_relaxation_fixpoint(num_v, num_e, directed,
                                                 seed):
    src, dst, w = graph(num_v, num_e, seed)
    got = sssp_oracle_f32(num_v, src, dst, w, 3, directed=directed)
    for order_seed in (1, 2):
        fix = stale_fixpoint(num_v, src, dst, w, 3, directed, order_seed)
        assert np.array_equal(got, fix)
    # every value is an fp32 value or DBL_MAX
    reached = got < 1e300
    assert np.array_equal(got[reached],
                          got[reached].astype(np.float32).astype(np.float64))
    assert got[3] == 0.0 and (got[num_v - 20:] == DBL_MAX).all()


@pytest.mark.parametrize("num_v,num_e,directed,seed", CASES)
def test_f32_dijkstra_near_fp64(num_v, num_e, directed, seed):
    src, dst, w = graph(num_v, num_e, seed)
    got = sssp_oracle_f32(num_v, src, dst, w, 3, directed=directed)
    exp = sssp_oracle(num_v, src, dst, w, 3, directed=directed)
    assert np.array_equal(got > 1e300, exp > 1e300)
    reached = exp < 1e300
    # a path of h arcs rounds h times, each by at most 2^-24 relative, on
    # partial sums that never exceed the total (weights are >= 0). hops is
    # the BFS depth of the farthest reached vertex. A lightest path may take
    # more arcs than the fewest-arc path, so this is tighter than the
    # worst case; it holds because the h roundings do not all align.
    depth = bfs_oracle(num_v, src, dst, 3, directed=directed)
    hops = int(depth[reached].max())
    assert hops >= 3
    err = np.abs(got[reached] - exp[reached])
    assert (err <= hops * 2.0 ** -24 * exp[reached]).all()
    # and the two really differ: the exact oracle is not the rounded fp64 one
    assert (got[reached] != exp[reached].astype(np.float32)).any()


def test_parallel_arcs_and_self_loops():
    # 0 -> 1 twice (5 then 2), self-loop on 1, 1 -> 2 of weight 0, 3 alone
    src = np.array([0, 0, 1, 1])
    dst = np.array([1, 1, 1, 2])
    w = np.array([5, 2, 1, 0], dtype=np.float32)
    got = sssp_oracle_f32(4, src, dst, w, 0, directed=True)
    assert got.tolist() == [0.0, 2.0, 2.0, DBL_MAX]
    got = sssp_oracle_f32(4, src, dst, w, 2, directed=True)
    assert got.tolist() == [DBL_MAX, DBL_MAX, 0.0, DBL_MAX]
    got = sssp_oracle_f32(4, src, dst, w, 2, directed=False)
    assert got.tolist() == [2.0, 0.0, 0.0, DBL_MAX]
