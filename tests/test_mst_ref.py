"""The fast host reference of test_gpu_mst_reference.py (mst_ref.distances_from_lcs, mst_ref.prim_edges_fast) against
the scalar forms it restates (mst_ref.pair_distances, mst_ref.prim_edges), bit for bit, on the degenerate sets a - h of
mst_shapes.py and both distance kinds.  No GPU."""
import numpy as np
import pytest

import mst_ref
import mst_shapes
from famsa_amd import seqio


def _same(a, b):
    return (a["from"] == b["from"]).all() and (a["to"] == b["to"]).all() and \
        (a["dist"].view(np.uint64) == b["dist"].view(np.uint64)).all()


@pytest.mark.parametrize("name", mst_shapes.CPU_SHAPES)
def test_fast_forms_equal_the_scalar_forms(oracle, name):
    seqs = mst_shapes.build(name)
    codes, offsets = seqio.pack(seqs)
    n = len(seqs)
    lens = np.diff(offsets.astype(np.int64))
    tri = oracle.triangle(codes, offsets)
    for kind in (1, 0):
        D = mst_ref.pair_distances(oracle, codes, offsets, kind)
        fast = mst_ref.distances_from_lcs(tri, lens, kind, oracle)
        assert fast.dtype == np.float64 and (fast.view(np.uint64) == D.view(np.uint64)).all(), (name, kind)
        # the square form reads its lower triangle only (ref = the larger id)
        sq = mst_ref.square_lcs(tri, n).astype(np.uint32)
        sq[np.triu_indices(n, 1)] = 7
        assert (mst_ref.distances_from_lcs(sq, lens, kind, oracle).view(np.uint64) == D.view(np.uint64)).all()
        want = mst_ref.prim_edges(D)
        assert _same(mst_ref.prim_edges_fast(D), want), (name, kind)
        rows = mst_ref.DistanceRows(mst_ref.square_lcs(tri, n), lens, kind, oracle)
        assert _same(mst_ref.prim_edges_fast(rows), want), (name, kind, "rows made as needed")


def test_zero_lcs_gives_the_largest_finite_double_but_one(oracle):
    D = mst_ref.distances_from_lcs(np.zeros(3, np.uint16), [0, 5, 0], 1, oracle)
    assert D[1, 0] == np.nextafter(np.finfo(np.float64).max, 0.0) == oracle.lib.oracle_dist_indel075_f64(0, 5, 0)
    assert (D.diagonal() == 0).all() and (D == D.T).all()


def test_the_id_order_alone_builds_the_tree_of_equal_distances(oracle):
    """All distances equal: from vertex 0 the largest packed pair wins each step -- (0, n-1) first, then (n-2, n-1), ..."""
    n = 6
    D = np.full((n, n), 2.0)
    np.fill_diagonal(D, 0.0)
    got = mst_ref.prim_edges_fast(D)
    assert _same(got, mst_ref.prim_edges(D))
    assert list(zip(got["from"], got["to"])) == [(0, 5), (4, 5), (3, 5), (2, 5), (1, 5)]
