"""The NumPy / Python-int oracle of the device random-walk sampler, and tests
of the oracle itself.

One 64-bit draw per step, a function of (seed, walk, hop) alone, walk being
the index into `starts` and hop the hop index of the vertex being left (all
arithmetic mod 2^64):

    x = seed*0x9E3779B97F4A7C15 + walk*0xD1B54A32D192ED03 + hop
    x ^= x>>30; x *= 0xBF58476D1CE4E5B9
    x ^= x>>27; x *= 0x94D049BB133111EB
    r = x ^ (x>>31)

index(r, n) = (r * n) >> 64. A row is the stored out-row of the vertex,
ascending destination id, deg its length:

  random       pick = index(r, deg)
  edge_weight  cdf = inclusive fp32 prefix sum of the row's weights,
               t = fp32(r >> 40) * 2^-24 * cdf[deg-1] (one fp32 multiply),
               pick = min(deg-1, #{i : cdf[i] <= t}); a total that is not > 0
               is a dead end
  top_k        kk = min(k, deg); pick = the index(r, kk)-th arc of the row
               ordered by weight descending, ties to the smaller slot

Without weights every weight is 1: edge_weight is then the random strategy and
top_k draws among the first kk slots.

The distribution checks below are properties of this generator for the named
seed (7, the default of Engine.sample), not of any code under test."""
import numpy as np

M64 = (1 << 64) - 1


def finalize(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, walk, hop):
    return finalize(seed * 0x9E3779B97F4A7C15 + walk * 0xD1B54A32D192ED03 +
                    hop)


def index(r, n):
    return (r * n) >> 64


def build_rows(num_v, src, dst, w=None, directed=True):
    """Stored out-rows: (off, dst, w) with every row ascending by destination
    (stable, so parallel arcs keep their input order: the device does not
    specify theirs). Undirected input is mirrored."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    if w is not None:
        w = np.asarray(w, dtype=np.float32)
    if not directed:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        if w is not None:
            w = np.concatenate([w, w])
    order = np.lexsort((dst, src))
    off = np.zeros(num_v + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_v), out=off[1:])
    return off, dst[order], None if w is None else w[order]


def pick_slot(r, w_row, deg, strategy, top_k):
    """The slot of the arc taken out of a row of deg >= 1 arcs, or None at a
    dead end. w_row: fp32 weights of the row, or None."""
    if strategy == "random" or (strategy == "edge_weight" and w_row is None):
        return index(r, deg)
    if strategy == "edge_weight":
        cdf = np.cumsum(w_row, dtype=np.float32)
        total = cdf[-1]
        if not total > 0:
            return None
        u = np.float32((r >> 40) * 2.0 ** -24)  # exact: 24 bits
        t = np.float32(u * total)  # fp32 * fp32, rounded to nearest
        return min(deg - 1, int(np.searchsorted(cdf, t, side="right")))
    assert strategy == "top_k"
    kk = min(top_k, deg)
    j = index(r, kk)
    if w_row is None or deg <= top_k:
        return j
    order = sorted(range(deg), key=lambda i: (-float(w_row[i]), i))
    return order[j]


def walk_oracle(num_v, src, dst, w, starts, hops, strategy="random", top_k=4,
                seed=7, directed=True):
    """(walk_ids, paths) of a world of one rank: every start that is a vertex
    gets a walk; -1 from the first dead end on."""
    off, adj, aw = build_rows(num_v, src, dst, w, directed)
    starts = np.asarray(starts, dtype=np.int64)
    walk_ids = np.nonzero((starts >= 0) & (starts < num_v))[0]
    paths = np.full((len(walk_ids), hops + 1), -1, dtype=np.int64)
    for row, walk in enumerate(walk_ids):
        v = int(starts[walk])
        paths[row, 0] = v
        for hop in range(hops):
            b, e = int(off[v]), int(off[v + 1])
            if e == b:
                break
            slot = pick_slot(draw(seed, int(walk), hop),
                             None if aw is None else aw[b:e], e - b, strategy,
                             top_k)
            if slot is None:
                break
            v = int(adj[b + slot])
            paths[row, hop + 1] = v
    return walk_ids.astype(np.int64), paths


# --- the generator ----------------------------------------------------------

def test_known_answers():
    # splitmix64 from state 0 returns finalize(1*g), finalize(2*g), ... with
    # g the golden-ratio increment; seed s, walk 0, hop 0 is finalize(s*g)
    assert draw(1, 0, 0) == 0xE220A8397B1DCDAF
    assert draw(2, 0, 0) == 0x6E789E6AA1B965F4
    assert draw(3, 0, 0) == 0x06C45D188009454F
    assert finalize(0) == 0
    # walk and hop enter the state before the finalizer
    assert draw(0, 0, 5) == finalize(5)
    assert draw(0, 1, 0) == finalize(0xD1B54A32D192ED03)
    assert draw(7, 3, 2) != draw(7, 2, 3)


def test_index_in_range():
    for n in (1, 2, 3, 63, 64, 65, 5000, (1 << 32) - 1, (1 << 40) + 7):
        assert index(0, n) == 0
        assert index(M64, n) == n - 1
        for s in range(50):
            assert 0 <= index(draw(s, s * 3, s % 5), n) < n
    assert index(1 << 63, 2) == 1 and index((1 << 63) - 1, 2) == 0


# --- distributions under the specified generator, seed 7 --------------------

def test_edge_weight_distribution():
    # weights 3 and 1 over 4096 one-hop walks: 3072 +- 5 sigma,
    # sigma = sqrt(4096 * 3/4 * 1/4) = 27.7
    src, dst = np.array([0, 0]), np.array([1, 2])
    w = np.array([3.0, 1.0], dtype=np.float32)
    _, paths = walk_oracle(3, src, dst, w, np.zeros(4096, dtype=np.int64), 1,
                           "edge_weight", seed=7)
    heavy = int((paths[:, 1] == 1).sum())
    assert int((paths[:, 1] == 2).sum()) == 4096 - heavy
    assert 2933 <= heavy <= 3211, heavy


def test_top_k_distribution():
    src = np.zeros(20, dtype=np.int64)
    dst = np.arange(1, 21, dtype=np.int64)
    w = np.arange(1, 21, dtype=np.float32)
    _, paths = walk_oracle(21, src, dst, w, np.zeros(4096, dtype=np.int64), 1,
                           "top_k", top_k=3, seed=7)
    vals, counts = np.unique(paths[:, 1], return_counts=True)
    assert vals.tolist() == [18, 19, 20]
    assert counts.min() >= 1000, counts


# --- walk semantics ---------------------------------------------------------

def test_dead_ends_unknown_starts_and_zero_hops():
    # 0 -> 1 -> 2, vertex 3 isolated
    src, dst = np.array([0, 1]), np.array([1, 2])
    ids, paths = walk_oracle(4, src, dst, None, [0, 9, 3, -1, 1, 0], 4)
    assert ids.tolist() == [0, 2, 4, 5]
    assert paths.tolist() == [[0, 1, 2, -1, -1], [3, -1, -1, -1, -1],
                              [1, 2, -1, -1, -1], [0, 1, 2, -1, -1]]
    ids, paths = walk_oracle(4, src, dst, None, [2, 0], 0)
    assert paths.tolist() == [[2], [0]]
    # a row whose weights sum to nothing is a dead end for edge_weight only
    w = np.array([0.0, 1.0], dtype=np.float32)
    _, paths = walk_oracle(4, src, dst, w, [0], 2, "edge_weight")
    assert paths.tolist() == [[0, -1, -1]]
    _, paths = walk_oracle(4, src, dst, w, [0], 2, "random")
    assert paths.tolist() == [[0, 1, 2]]


def test_unweighted_edge_weight_is_random_and_ties_take_slot_order():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 50, 600)
    dst = rng.integers(0, 50, 600)
    starts = rng.integers(0, 50, 100)
    a = walk_oracle(50, src, dst, None, starts, 3, "edge_weight", seed=5)
    b = walk_oracle(50, src, dst, None, starts, 3, "random", seed=5)
    assert np.array_equal(a[1], b[1])
    # equal weights: the order is the slot order, so top_k over a weighted
    # row of ties is top_k over the unweighted row
    ones = np.ones(600, dtype=np.float32)
    c = walk_oracle(50, src, dst, ones, starts, 3, "top_k", top_k=2, seed=5)
    d = walk_oracle(50, src, dst, None, starts, 3, "top_k", top_k=2, seed=5)
    assert np.array_equal(c[1], d[1])
    off, adj, _ = build_rows(50, src, dst)
    for path in c[1]:
        for h in range(3):
            if path[h + 1] >= 0:
                row = adj[off[path[h]]:off[path[h] + 1]]
                assert path[h + 1] in row[:2]


def test_undirected_rows_are_mirrored_and_sorted():
    off, adj, w = build_rows(4, [2, 0, 3], [0, 1, 0],
                             np.array([1, 2, 3], dtype=np.float32),
                             directed=False)
    assert off.tolist() == [0, 3, 4, 5, 6]
    assert adj.tolist() == [1, 2, 3, 0, 0, 0]
    assert w.tolist() == [2, 1, 3, 2, 1, 3]
