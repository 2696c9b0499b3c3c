"""The exact k-NN in numpy, shared by the k-NN tests and the planner batch's reference."""
import numpy as np


def knn_ref(nodes, k, max_dist=0.0):
    """(n, k) neighbour indices: distance (dx^2 + dy^2) + dz^2, then lower index; self
    excluded; -1 where fewer than k exist (within max_dist, exclusive, when > 0)."""
    n = len(nodes)
    out = np.full((n, k), -1, np.int32)
    r2 = max_dist * max_dist if max_dist > 0 else 1e300
    for i in range(n):
        d = nodes - nodes[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = np.nonzero((d2 < r2) & (np.arange(n) != i))[0]
        order = cand[np.lexsort((cand, d2[cand]))][:k]  # distance, then lower index
        out[i, :len(order)] = order
    return out


def knn_row(nodes, i, k):
    """Row i of knn_ref(nodes, k) and the squared distances to every node."""
    d = nodes - nodes[i]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    cand = np.nonzero(np.arange(len(nodes)) != i)[0]
    order = cand[np.lexsort((cand, d2[cand]))][:k]
    row = np.full(k, -1, np.int32)
    row[:len(order)] = order
    return row, d2
