"""Dense k-clique counts for k in {2, 3, 4} on a boolean adjacency matrix,
held equal to oracles.kclique_oracle. The matrix products run in float64 and
stay exact: every entry and every partial sum is an integer far below 2^53
at the sizes the tests use. tests/test_gpu_kclique.py imports kclique_dense
for graphs too large for the recursive oracle."""
import numpy as np

from oracles import kclique_oracle


def dense_adjacency(num_v, src, dst):
    """Simple undirected adjacency: duplicates and self-loops dropped."""
    A = np.zeros((num_v, num_v), dtype=bool)
    A[src, dst] = True
    A[dst, src] = True
    np.fill_diagonal(A, False)
    return A


def kclique_dense(A, k):
    A = np.asarray(A, dtype=bool)
    F = A.astype(np.float64)
    if k == 2:
        return int(A.sum()) // 2
    if k == 3:
        tr = np.trace(F @ F @ F)
        assert tr < 2.0 ** 53
        return int(round(tr)) // 6
    if k == 4:
        # every 4-clique is met once, from its lowest id: the triangles among
        # the neighbours of v with a higher id
        total = 0
        for v in range(A.shape[0]):
            hi = np.flatnonzero(A[v, v + 1:]) + v + 1
            if len(hi) < 3:
                continue
            S = F[np.ix_(hi, hi)]
            tr = np.einsum("ij,ji->", S @ S, S)  # trace(S^3)
            assert tr < 2.0 ** 53
            total += int(round(tr)) // 6
        return total
    raise ValueError("kclique_dense: k in {2, 3, 4}")


def gnp_upper(n, p, seed):
    """Edges of G(n, p) from an upper-triangular Bernoulli draw."""
    rng = np.random.default_rng(seed)
    src, dst = np.nonzero(np.triu(rng.random((n, n)) < p, 1))
    return src.astype(np.int64), dst.astype(np.int64)


def test_dense_equals_oracle_gnp():
    src, dst = gnp_upper(40, 0.5, seed=3)
    A = dense_adjacency(40, src, dst)
    for k in (2, 3, 4):
        assert kclique_dense(A, k) == kclique_oracle(40, src, dst, k), k


def test_dense_ignores_duplicates_and_loops():
    src = np.array([0, 0, 1, 1, 2, 2, 3], dtype=np.int64)
    dst = np.array([1, 1, 0, 2, 0, 2, 3], dtype=np.int64)
    A = dense_adjacency(4, src, dst)
    assert kclique_dense(A, 2) == 3
    assert kclique_dense(A, 3) == 1
    assert kclique_dense(A, 4) == 0


def test_dense_complete_graph():
    A = ~np.eye(9, dtype=bool)
    assert [kclique_dense(A, k) for k in (2, 3, 4)] == [36, 84, 126]
