"""tests/upgma_ref.py -- the numpy restatement of UPGMA::computeTree that the tests of lcsgpu_upgma_batch compare against --
pinned here, without a GPU: its trees, rendered with the host layer's Newick writer over the host layer's working order,
must equal Host.tree_from_matrix (pinned to the reference by test_differential.py) and, where oracle/_ref is built, the
reference's own text.  Tie-heavy random sets (small alphabets: many equal float distances, so every '<' and every stale
minimum decides something) of 2, 3, 40, 257 and 700 sequences, both distances, both averages; and one set without a finite
nearest neighbour (zero_last: a block of empty sequences), where the helper must say so at the step the host builder
refuses."""
import os

import numpy as np
import pytest

import mst_shapes
import oracle_bind
import upgma_ref
from famsa_amd import hostlib as host_bind
from famsa_amd import seqio

SETS = [(2, 5, "AC"), (3, 8, "AC"), (40, 12, "AC"), (257, 20, "ACD"), (700, 60, "ACDE")]
DISTS = [(1, "indel075_div_lcs"), (0, "indel_div_lcs")]


@pytest.fixture(scope="module")
def host():
    return host_bind.Host()


def tie_heavy(seed, n, max_len, alpha):
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    return ["".join(alpha[i] for i in rng.integers(0, len(alpha), size=int(rng.integers(1, max_len + 1)))) + "A" for _ in range(n)]


def unique_order(host, fasta, n):
    """(records of the unique sequences in working order, sorted2input, sorted2unique)"""
    u, s2i, s2u = host.workset(fasta, n)
    first = np.full(u, -1, np.int64)
    for k in range(n - 1, -1, -1):
        first[s2u[k]] = k
    return s2i[first], s2i, s2u


def helper_newick(host, oracle, fasta, names, lens, sq, kind, modified):
    """The helper's tree of a file as Newick bytes, or None when the helper finds no finite nearest neighbour."""
    n = len(names)
    in_of, s2i, s2u = unique_order(host, fasta, n)
    if len(in_of) < 2:
        return b""
    D = upgma_ref.dist_square(oracle, sq[np.ix_(in_of, in_of)], lens[in_of], kind)
    left, right, ok = upgma_ref.upgma_tree(D, modified)
    if not ok:
        return None
    return host.newick(left, right, [names[i] for i in s2i], sorted2unique=s2u)


@pytest.mark.parametrize("seed", range(len(SETS)))
def test_helper_equals_the_host_builder_and_the_reference(host, oracle, tmp_path, seed):
    n, max_len, alpha = SETS[seed]
    seqs = tie_heavy(seed, n, max_len, alpha)
    names = ["r%d" % i for i in range(n)]
    fasta = str(tmp_path / "in.fasta")
    with open(fasta, "w") as f:
        for name, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (name, s))
    enc = [oracle.encode(s) for s in seqs]
    codes, offsets = seqio.pack(enc)
    lens = np.array([len(e) for e in enc], np.uint32)
    sq = oracle.rect(codes, offsets, np.arange(n), np.arange(n))
    ref = oracle_bind.Ref() if oracle_bind.have_ref() else None
    h = ref.open_fasta(fasta) if ref else None
    try:
        for kind, dist in DISTS:
            for gt in ("upgma", "upgma_modified"):
                got = helper_newick(host, oracle, fasta, names, lens, sq, kind, gt == "upgma_modified")
                assert got == host.tree_from_matrix(fasta, sq, gt, distance=dist), (dist, gt)
                if ref:
                    assert got == ref.tree(h, gt, distance=kind, threads=2), (dist, gt)
    finally:
        if ref:
            ref.close(h)


@pytest.mark.parametrize("gt", ["upgma", "upgma_modified"])
def test_a_set_without_a_finite_nearest_neighbour(host, oracle, tmp_path, gt):
    """zero_last: the empty sequence has LCS 0 with everybody, so once everything else is one cluster no row has a key
    below BIG_DIST -- the host builder refuses the file, and the helper reports not ok."""
    fasta = str(tmp_path / "zero_last.fasta")
    mst_shapes.write_zero_last_fasta(fasta)
    enc = mst_shapes.build("zero_last")
    n = len(enc)
    codes, offsets = seqio.pack(enc)
    lens = np.array([len(e) for e in enc], np.uint32)
    sq = oracle.rect(codes, offsets, np.arange(n), np.arange(n))
    for kind, dist in DISTS:
        assert helper_newick(host, oracle, fasta, ["s%d" % i for i in range(n)], lens, sq, kind, gt == "upgma_modified") is None
        with pytest.raises(RuntimeError, match="no finite nearest neighbour"):
            host.tree_from_matrix(fasta, sq, gt, distance=dist)
