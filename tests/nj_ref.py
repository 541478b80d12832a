"""Test infrastructure: NeighborJoining::computeTree (reference tree/NeighborJoining.cpp:33-118) restated in numpy float32,
one matrix operation per merge, over a square float32 matrix (upgma_ref.dist_square: pair (i, j) takes the value with the
later member as the ref, calculateDistanceMatrix's orientation).  One float32 rounding per operation:
q = ((live - 2) * D - sum_i) - sum_j, the first strict minimum below FLT_MAX over i < j in the order of the live clusters
(a NaN never wins; np.argmin would pick one, so the candidates are filtered with '<' first); sum_k -= (Dik + Djk);
Dik = (Dik + Djk - Dij) / 2; sum_k += Dik; the merged cluster's sum the new Dik one after the other in ascending k
(np.cumsum in float32 is sequential, np.sum is not).  The live clusters stay in ascending row order and the merged cluster
keeps its left child's place, so the matrix is simply kept compact.  A helper for the tests of lcsgpu_nj_batch, pinned by
test_nj_ref.py; nothing in famsa_amd/ imports this."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def nj_tree(D):
    """(left, right, ok): children of the internal nodes m .. 2m - 2 in the order they are made.  ok = False when a merge
    finds no q below FLT_MAX -- where the reference keeps min_i = min_j = 0 and its result is degenerate; the records from
    that merge on are unspecified.  D is not changed."""
    D = np.array(D, np.float32, copy=True)
    m = len(D)
    left, right = np.zeros(max(m - 1, 0), np.int32), np.zeros(max(m - 1, 0), np.int32)
    if m < 2:
        return left, right, True
    np.fill_diagonal(D, np.float32(0))  # + 0.0f changes no float sum that started at + 0.0f
    two = np.float32(2)
    with np.errstate(over="ignore", invalid="ignore"):  # FLT_MAX + FLT_MAX = +inf, inf - inf = NaN, as in the reference
        s = np.cumsum(D, axis=1, dtype=np.float32)[:, -1].copy()
        node = np.arange(m)
        not_above = ~np.triu(np.ones((m, m), bool), 1)  # (a leading block of it is the same mask of a smaller matrix)
        step = 0
        while len(D) > 2:
            live = len(D)
            q = np.float32(live - 2) * D
            q -= s[:, None]
            q -= s[None, :]
            q[~(q < FLT_MAX)] = np.inf  # NaN included
            q[not_above[:live, :live]] = np.inf
            at = int(q.argmin())  # row-major: the first minimum in (i, j) lexicographic order
            i, j = divmod(at, live)
            if not q[i, j] < FLT_MAX:
                return left, right, False
            left[step], right[step] = node[i], node[j]
            node[i] = m + step
            others = np.ones(live, bool)
            others[i] = others[j] = False
            u = D[i] + D[j]
            new = (u - D[i, j]) / two
            s = np.where(others, (s - u) + new, s)
            new = np.where(others, new, np.float32(0))
            s[i] = np.cumsum(new, dtype=np.float32)[-1]
            D[i, :] = new
            D[:, i] = new
            D = np.delete(np.delete(D, j, 0), j, 1)
            s = np.delete(s, j)
            node = np.delete(node, j)
            step += 1
    left[step], right[step] = node[0], node[1]
    return left, right, True
