"""tests/nj_ref.py -- the numpy restatement of NeighborJoining::computeTree that the tests of lcsgpu_nj_batch compare against --
pinned here, without a GPU: its trees, rendered with the host layer's Newick writer over the host layer's working order,
must equal Host.tree_from_matrix(..., "nj") (pinned to the reference by test_differential.py) and, where oracle/_ref is
built, the reference's own text.  The tie-heavy random sets of test_upgma_ref.py (small alphabets: many equal float
distances, so the order of every '<' and of every float sum decides something) of 2, 3, 40, 257 and 700 sequences, both
distances; and sets without a finite q (allx: sequences of the code that matches nothing; zero_scattered: empty sequences
all over), where the helper must say so and the host builder, asked to treat the matrix as a whole input
(FAMSA_HOST_TEST=matrix_whole_input, the way a batch chunk hands it a file), refuses in the device reducer's words."""
import numpy as np
import pytest

import mst_shapes
import nj_ref
import oracle_bind
import upgma_ref
from famsa_amd import hostlib as host_bind
from famsa_amd import seqio
from test_upgma_ref import DISTS, SETS, tie_heavy, unique_order


@pytest.fixture(scope="module")
def host():
    return host_bind.Host()


def helper_newick(host, oracle, fasta, names, lens, sq, kind):
    """The helper's tree of a file as Newick bytes, or None when the helper finds no q below FLT_MAX at some merge."""
    n = len(names)
    in_of, s2i, s2u = unique_order(host, fasta, n)
    if len(in_of) < 2:
        return b""
    D = upgma_ref.dist_square(oracle, sq[np.ix_(in_of, in_of)], lens[in_of], kind)
    left, right, ok = nj_ref.nj_tree(D)
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
            got = helper_newick(host, oracle, fasta, names, lens, sq, kind)
            assert got is not None, dist
            assert got == host.tree_from_matrix(fasta, sq, "nj", distance=dist), dist
            if ref:
                assert got == ref.tree(h, "nj", distance=kind, threads=2), dist
    finally:
        if ref:
            ref.close(h)


def test_the_helper_does_not_change_its_input(oracle):
    rng = np.random.Generator(np.random.PCG64(9))
    D = rng.integers(1, 9, size=(30, 30)).astype(np.float32)
    D = np.triu(D, 1) + np.triu(D, 1).T
    before = D.copy()
    left, right, ok = nj_ref.nj_tree(D)
    assert ok and (D == before).all() and len(left) == len(right) == 29
    assert sorted(np.concatenate([left, right]).tolist()) == list(range(58))  # every node but the root is a child once


def test_nan_never_wins():
    """Rows 0 and 1 are at FLT_MAX from everybody, so every sum is +inf: a pair at FLT_MAX has q = inf - inf = NaN, the pair
    (2, 3) has q = -inf and is the first strict minimum -- np.argmin alone would have picked the NaN of (0, 1)."""
    big = nj_ref.FLT_MAX
    D = np.array([[0, big, big, big], [big, 0, big, big], [big, big, 0, 1], [big, big, 1, 0]], np.float32)
    left, right, ok = nj_ref.nj_tree(D)
    assert not ok  # after (2, 3) no q is below FLT_MAX
    assert (left[0], right[0]) == (2, 3)


@pytest.mark.parametrize("shape", ["allx", "zero_scattered"])
def test_sets_without_a_finite_q(host, oracle, tmp_path, monkeypatch, shape):
    enc = mst_shapes.build(shape)
    n = len(enc)
    fasta = str(tmp_path / (shape + ".fasta"))
    with open(fasta, "w") as f:
        for i, s in enumerate(enc):  # (the empty sequences are gap-only records: the reader keeps them as length 0)
            f.write(">s%d\n%s\n" % (i, "".join(seqio.ALPHABET[c] for c in s) if len(s) else "-"))
    codes, offsets = seqio.pack(enc)
    lens = np.array([len(e) for e in enc], np.uint32)
    sq = oracle.rect(codes, offsets, np.arange(n), np.arange(n))
    monkeypatch.setenv("FAMSA_HOST_TEST", "matrix_whole_input")
    for kind, dist in DISTS:
        assert helper_newick(host, oracle, fasta, ["s%d" % i for i in range(n)], lens, sq, kind) is None
        with pytest.raises(RuntimeError, match="NJ: no finite q"):
            host.tree_from_matrix(fasta, sq, "nj", distance=dist)
