"""The long branch of every batched call.  A single member beyond 2048 residues sends every list of a batched call down a
list-by-list (or evaluation-by-evaluation) branch of csrc/lcsgpu_fasttree.hip -- the long-ref kernel keeps its 2-D grid -- with
its own synchronisation and its own accounting of the kernel time: lcsgpu_mst_prim_batch, lcsgpu_upgma_batch and lcsgpu_nj_batch
through GroupCall (had_long), lcsgpu_assign_seeds_batch (any_long), lcsgpu_clarans_batch, and `famsa-gpu -gt ... -batch` with a
file that has long members.

One set is uploaded for the whole file: a 20-letter family of 150 members of 60..300 residues, 12 plain long members of
2100..4200 residues (half of them mutated copies of one parent, so that trees have structure) and 3 orientation-sensitive long
members of test_gpu_lcs_long.py's recipe.  Its square of LCS values comes from the oracle once; the expected records come from
the independent references of the short routes' tests (mst_ref, upgma_ref, nj_ref, the host sweep, the CLARANS searcher).
After each long call a call of the same kind without any long member runs on the same engine: it must still be exact, and
last_kernel_ms() must be finite and positive for both.  All comparisons are exact."""
import math
import os

import numpy as np
import pytest

import mst_ref
import nj_ref
import test_gpu_batch_trees as bt
import test_gpu_lcs_long as lcs_long
import upgma_ref
from famsa_amd import hostlib as host_bind
from famsa_amd import seqio
from famsa_amd.lcsgpu import MST_EDGE
from test_gpu_clarans import searcher  # noqa: F401
from test_gpu_mst_batch import _first_difference, _same

pytestmark = pytest.mark.gpu
N_FAMILY, N_LONG, N_QUIRK = 150, 12, 3
F = np.arange(N_FAMILY, dtype=np.int32)
L = np.arange(N_FAMILY, N_FAMILY + N_LONG, dtype=np.int32)
Q = np.arange(N_FAMILY + N_LONG, N_FAMILY + N_LONG + N_QUIRK, dtype=np.int32)
_SET = {}


def _make_set():
    rng = np.random.default_rng(20490)
    parent = rng.integers(0, 20, size=300).astype(np.uint8)
    seqs = []
    for _ in range(N_FAMILY):
        s = parent[:int(rng.integers(60, 301))].copy()
        m = rng.random(len(s)) < rng.uniform(0.05, 0.4)
        s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
        seqs.append(s)
    long_parent = rng.integers(0, 20, size=4200).astype(np.uint8)
    for k in range(N_LONG):
        length = [2100, 4200][k] if k < 2 else int(rng.integers(2100, 4201))
        s = rng.integers(0, 20, size=length).astype(np.uint8)
        if k % 2 == 0:
            keep = rng.random(length) >= rng.choice([0.1, 0.3])
            s[keep] = long_parent[:length][keep]
        seqs.append(s)
    # a homopolymer word at the last word of a pass and the first of the next (33 words), at 31 | 32 (41 words), at 1, 16, 32 (70)
    picks = [lcs_long.QUIRK_WORDS.index(w) * len(lcs_long.QUIRK_AT) + lcs_long.QUIRK_AT.index(at) for w, at in ((33, (15, 16)), (41, (31, 32)), (70, (1, 16, 32)))]
    seqs += [lcs_long.QUIRK[p] for p in picks]
    assert len(seqs) == N_FAMILY + N_LONG + N_QUIRK and len({s.tobytes() for s in seqs}) == len(seqs)
    return seqs


def _the_set(oracle):
    """(sequences, lengths, sq): sq[ref, partner] over the whole set from the oracle -- computed once, read-only."""
    if not _SET:
        seqs = _make_set()
        codes, offsets = seqio.pack(seqs)
        n = len(seqs)
        sq = oracle.rect(codes, offsets, np.arange(n), np.arange(n))
        assert (sq > 0).all()  # every pair has a finite distance: every group has a UPGMA and an NJ tree
        assert (sq[:Q[0], :Q[0]] == sq[:Q[0], :Q[0]].T).all() and all((sq[q] != sq[:, q]).any() for q in Q)
        sq.flags.writeable = False
        _SET.update(seqs=seqs, lens=np.array([len(s) for s in seqs], np.int64), sq=sq)
    return _SET["seqs"], _SET["lens"], _SET["sq"]


@pytest.fixture(scope="module")
def loaded(engine, oracle):
    seqs, lens, sq = _the_set(oracle)
    engine.upload_seqs(seqs)
    flags = engine.orientation_flags()
    assert flags[Q].all() and flags.sum() == N_QUIRK
    return engine


EMPTY, ONE = np.zeros(0, np.int32), F[5:6]
WITH_QUIRK = np.concatenate([F[70:90], Q[:1], L[2:5], Q[1:]]).astype(np.int32)
# long members, none of them orientation sensitive: the first member, the last, every member; beside them groups without a
# long member (they take the list-by-list branch too), an empty and a one-member group
PLAIN_GROUPS = [np.concatenate([L[:1], F[:30]]), EMPTY, np.concatenate([F[30:70], L[1:2]]), ONE, L, F[:70], F[100:102],
                np.concatenate([F[110:120], L[5:9], F[120:125]])]
QUIRK_GROUPS = [WITH_QUIRK, F[90:100], WITH_QUIRK[::-1].copy(), ONE, np.concatenate([Q, L[9:]])]
SHORT_GROUPS = [F[:70], EMPTY, F[100:102], ONE, F[60:125][::-1].copy()]
assert all(len(g) <= 70 for g in PLAIN_GROUPS + QUIRK_GROUPS + SHORT_GROUPS)


def _kernel_ms(engine):
    ms, launches = engine.last_kernel_ms()
    assert math.isfinite(ms) and ms > 0 and launches > 0, (ms, launches)


def _list_square(ids):
    return _SET["sq"][np.ix_(ids, ids)]  # [k, c] = LCS(ref = list[k], partner = list[c])


# ---- lcsgpu_mst_prim_batch ----------------------------------------------------------------------------------------------------

def _check_mst(engine, oracle, groups, kind, flag):
    got = engine.mst_prim_batch(groups, kind=kind, triangle_orientation=flag)
    _kernel_ms(engine)
    assert len(got) == len(groups)
    bad = []
    for g, ids in zip(got, groups):
        if len(ids) < 2:
            want = np.zeros(0, MST_EDGE)
        else:  # as test_gpu_mst_batch._want: the triangle's orientation (ref = the later member), the list's own order
            rows = mst_ref.DistanceRows(mst_ref.square_lcs(_list_square(ids), len(ids)), _SET["lens"][ids], kind, oracle)
            want = mst_ref.prim_edges_fast(rows)
        if not _same(g, want):
            bad.append((len(ids), _first_difference(g, want)))
    assert not bad, (kind, flag, bad)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_mst_prim_batch(loaded, oracle, kind, flag):
    """With LCSGPU_MST_TRIANGLE_ORIENTATION the orientation-sensitive long members are served too, forwards and reversed."""
    _check_mst(loaded, oracle, PLAIN_GROUPS + (QUIRK_GROUPS if flag else []), kind, flag)
    _check_mst(loaded, oracle, SHORT_GROUPS, kind, flag)


# ---- lcsgpu_upgma_batch, lcsgpu_nj_batch -------------------------------------------------------------------------------------------

def _check_trees(engine, oracle, groups, kind, call, reference):
    trees, status = call(groups)
    _kernel_ms(engine)
    assert len(trees) == len(groups) and len(status) == len(groups)
    bad = []
    for g, (ids, (left, right)) in enumerate(zip(groups, trees)):
        if len(ids) < 2:
            wl = wr = np.zeros(0, np.int32)
        else:
            wl, wr, ok = reference(upgma_ref.dist_square(oracle, _list_square(ids), _SET["lens"][ids].astype(np.uint32), kind))
            assert ok, (g, "the reference builds no tree here")  # (must_build)
        if int(status[g]) != 0 or len(left) != len(wl) or (left != wl).any() or (right != wr).any():
            bad.append((g, len(ids), int(status[g])))
    assert not bad, (kind, bad)


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_upgma_batch(loaded, oracle, kind, modified):
    for groups in (PLAIN_GROUPS + QUIRK_GROUPS, SHORT_GROUPS):
        _check_trees(loaded, oracle, groups, kind, lambda g: loaded.upgma_batch(g, kind=kind, modified=modified),
                     lambda D: upgma_ref.upgma_tree(D, modified))


@pytest.mark.parametrize("kind", [1, 0])
def test_nj_batch(loaded, oracle, kind):
    for groups in (PLAIN_GROUPS + QUIRK_GROUPS, SHORT_GROUPS):
        _check_trees(loaded, oracle, groups, kind, lambda g: loaded.nj_batch(g, kind=kind), nj_ref.nj_tree)


# ---- lcsgpu_assign_seeds_batch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [1, 0])
def test_assign_seeds_batch(loaded, oracle, kind):
    """Three evaluations, one with a long seed and one with a long seed that is orientation sensitive (and one without: it runs
    evaluation by evaluation too), against the host sweep -- the first seed's row, then strict '<' in seed order -- over the
    oracle's float distances; then three evaluations without a long seed."""
    _, lens, sq = _the_set(oracle)
    n = len(lens)
    fn = oracle.lib.oracle_dist_indel075_f32 if kind == 1 else oracle.lib.oracle_dist_indel_f32
    rng = np.random.default_rng(20491 + kind)
    short_seeds = [rng.permutation(F)[:m].astype(np.int32) for m in (13, 9, 17)]
    long_seeds = [short_seeds[0], np.insert(short_seeds[1], 4, L[3]).astype(np.int32), np.concatenate([Q[1:2], short_seeds[2], L[7:8]]).astype(np.int32)]
    cols = [rng.integers(0, n, size=m).astype(np.int32) for m in (300, 257, 120)]  # (long columns among them)
    for seeds in (long_seeds, short_seeds):
        got_d, got_a = loaded.assign_seeds_batch(seeds, cols, kind=kind)
        _kernel_ms(loaded)
        for g in range(3):
            d = np.array([[fn(int(sq[s, c]), int(lens[s]), int(lens[c])) for c in cols[g]] for s in seeds[g]], np.float32)
            want_a = d.argmin(axis=0).astype(np.int32)  # the first of equal minima: what strict '<' in seed order keeps
            want_d = d[want_a, np.arange(d.shape[1])]
            assert (got_a[g] == want_a).all(), (kind, g, int((got_a[g] != want_a).sum()))
            assert (got_d[g].view(np.uint32) == want_d.view(np.uint32)).all(), (kind, g)


# ---- lcsgpu_clarans_batch ----------------------------------------------------------------------------------------------------------

def test_clarans_batch(loaded, oracle, searcher):
    """Two samples, one with long members (an orientation-sensitive one among them), against the searcher of
    test_gpu_clarans.py on the oracle's float triangle; then two samples without a long member."""
    _, lens, sq = _the_set(oracle)
    rng = np.random.default_rng(20493)
    with_long = np.sort(np.concatenate([rng.permutation(F)[:80], L[[0, 4, 6, 10]], Q[2:]])).astype(np.int32)
    short = [np.sort(rng.permutation(F)[:m]).astype(np.int32) for m in (60, 45)]
    for samples, ks in (([with_long, short[0]], [8, 6]), (short, [6, 5])):
        got = loaded.clarans_batch(samples, ks, 1, 0.1, 2)
        _kernel_ms(loaded)
        for ids, k, medoids in zip(samples, ks, got):
            ii, jj = np.tril_indices(len(ids), -1)  # row-major over the lower triangle: ref = the later member
            tri = oracle.dist_triangle_f32(sq[ids[ii], ids[jj]], lens[ids].astype(np.uint32), 1)
            assert medoids.tolist() == searcher(tri, len(ids), k, 1, 0.1, 2).tolist(), (len(ids), k)


# ---- famsa-gpu -gt ... -gt_export -batch ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fasta_files(tmp_path_factory, oracle):
    """Three small FASTA files, the second with long members (none orientation sensitive: -gt sl keeps such a file out of the
    batch), and their oracle squares in file order."""
    seqs, _, sq = _the_set(oracle)
    d = tmp_path_factory.mktemp("long_routes")
    out = []
    for name, ids in (("short40", F[:40]), ("with_long", np.concatenate([F[40:52], L[:2], F[52:65], L[4:6]])), ("short12", F[130:142])):
        path = str(d / (name + ".fasta"))
        with open(path, "w") as f:
            for i in ids:
                f.write(">%s_%d\n%s\n" % (name, i, "".join(seqio.ALPHABET[c] for c in seqs[i])))
        out.append((path, np.ascontiguousarray(sq[np.ix_(ids, ids)], np.uint32)))
    return out


@pytest.mark.parametrize("gt", ["sl", "upgma", "nj"])
def test_cli_batch_with_a_long_file(fasta_files, tmp_path, gt):
    """Every tree byte-equal to the host builder over the oracle's square (pinned to the reference by the CPU suite); all three
    files run inside the batch, the merges of UPGMA and NJ on the device."""
    lst, outs = bt._write_list(tmp_path, [path for path, _ in fasta_files], gt)
    p = bt._run(["-gt", gt, "-gt_export", "-batch", lst, "-v"])
    assert p.returncode == 0 and "[ERROR]" not in p.stderr, p.stderr[-2000:]
    host = host_bind.Host()
    for (path, square), out in zip(fasta_files, outs):
        assert open(out, "rb").read() == host.tree_from_matrix(path, square, gt), os.path.basename(path)
    t = {k: int(v) for k, v in bt._totals(p.stderr).items() if k.startswith("batch.")}
    assert t["batch.files"] == 3 and t["batch.files_failed"] == 0
    assert t["batch.files_in_chunks"] == 3 and t["batch.files_one_file_route"] == 0, t
    if gt != "sl":
        assert t["batch.files_device_" + gt] == 3, t
