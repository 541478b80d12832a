"""lcsgpu_upgma_batch -- UPGMA of many id lists of one uploaded set, one workgroup per list -- against a reference that
is NOT the engine: UPGMA::computeTree in numpy float32 (upgma_ref.upgma_tree, pinned by test_upgma_ref.py) over the
oracle's distances of the oracle's LCS values, list by list, in the list's own order and with the triangle's orientation
(ref = the later member).  One set is uploaded for the whole file: the set of test_gpu_mst_batch.py (the degenerate sets
of mst_shapes.py, 4096 short random sequences, the orientation-sensitive sequences of tests/golden/adversarial_tree.fasta)
and behind it a hub family of 300 (every member the hub with a few substitutions: one cluster that swallows a row per
merge, so the same matrix row is re-created step after step) and 4096 random sequences over four letters (`dense`: every
pair has a common residue, and equal distances abound).

A pair with LCS 0 has the distance FLT_MAX, and so has every cluster that holds one of the two to every cluster that holds
the other: such a set ends without a finite nearest neighbour unless stale minima happen to carry it through.  That is
the fate of most size groups cut from test_gpu_mst_batch.py's set (short sequences over 20 letters) and of `ties` (AAA
against CCC) -- there the status must say so, as the reference does -- so every size is also run on a cut of `dense`,
where the reference builds a tree and all m - 1 records are compared.

Group sizes: 0 and 1 (no record), 2 and 3, 63 / 64 / 65 (a wave), 255 / 256 / 257 (the stride of the 256-thread workgroup),
1023 / 1024 / 1025 (the stride of the 1024-thread workgroup, and the size from which a launch uses it), 4096 (the cap).
left / right are compared exactly; status must be `not ok` of the reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import famsa_amd
import mst_shapes
import test_gpu_mst_batch as mst_batch
import upgma_ref
from famsa_amd.lcsgpu import UPGMA_BATCH_MAX_MEMBERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = ["ties", "duplicates", "prefixes"]
MAYBE = ["zero_only", "allx", "zero_scattered"]
SIZES = mst_batch.SIZES
_size_group = mst_batch._size_group
_SET = {}
_LCS = {}
_REF = {}


def _the_set(oracle):
    """(sequences, {name: id range}): test_gpu_mst_batch's set and the hub family -- built once."""
    if not _SET:
        from famsa_amd import seqio
        seqs, where = mst_batch._the_set(oracle)
        seqs, where = list(seqs), dict(where)
        rng = np.random.Generator(np.random.PCG64(61))  # the `hub` recipe of test_gpu_endtoend.py, 300 members
        hub = rng.integers(0, 20, size=120, dtype=np.uint8)
        part = [hub]
        for _ in range(299):
            s = hub.copy()
            m = rng.random(120) < rng.uniform(0.02, 0.3)
            s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
            part.append(s)
        where["hub"] = np.arange(len(seqs), len(seqs) + len(part), dtype=np.int32)
        seqs += part
        part = mst_shapes._random(np.random.Generator(np.random.PCG64(4096)), 12, 40, UPGMA_BATCH_MAX_MEMBERS, letters=4)
        where["dense"] = np.arange(len(seqs), len(seqs) + len(part), dtype=np.int32)
        seqs += part
        _SET["seqs"], _SET["where"] = seqs, where
        _SET["packed"] = seqio.pack(seqs)
        _SET["lens"] = np.array([len(s) for s in seqs], np.uint32)
    return _SET["seqs"], _SET["where"]


def _distances(oracle, ids, kind):
    ids = np.asarray(ids, np.int32)
    key = ids.tobytes()
    if key not in _LCS:  # (both kinds and both averages share the LCS values)
        codes, offsets = _SET["packed"]
        _LCS[key] = oracle.rect(codes, offsets, ids, ids)  # [k, c] = LCS(ref = list[k], partner = list[c])
    return upgma_ref.dist_square(oracle, _LCS[key], _SET["lens"][ids], kind)


def _want(oracle, ids, kind, modified):
    """The reference's (left, right, ok) of one id list: computed once per (list, kind, average), shared read-only."""
    key = (np.asarray(ids, np.int32).tobytes(), kind, bool(modified))
    if key not in _REF:
        if len(ids) < 2:
            want = (np.zeros(0, np.int32), np.zeros(0, np.int32), True)
        else:
            want = upgma_ref.upgma_tree(_distances(oracle, ids, kind), modified)
        want[0].flags.writeable = False
        want[1].flags.writeable = False
        _REF[key] = want
    return _REF[key]


def _compare(oracle, groups, trees, status, kind, modified, must_build=False):
    assert len(trees) == len(groups) and len(status) == len(groups)
    bad = []
    for g, (ids, (left, right)) in enumerate(zip(groups, trees)):
        wl, wr, ok = _want(oracle, ids, kind, modified)
        if must_build and not ok:
            bad.append((g, len(ids), "the reference builds no tree here"))
        elif int(status[g]) != (0 if ok else 1):
            bad.append((g, len(ids), "status %d, reference ok = %s" % (status[g], ok)))
        elif ok and not (len(left) == len(wl) and (left == wl).all() and (right == wr).all()):
            k = int(np.flatnonzero((left != wl) | (right != wr))[0]) if len(left) == len(wl) else -1
            bad.append((g, len(ids), "node %d: got (%d, %d), want (%d, %d)" % (k, left[k], right[k], wl[k], wr[k]) if k >= 0
                        else "%d records, want %d" % (len(left), len(wl))))
    assert not bad, (kind, modified, bad)


def _check(engine, oracle, groups, kind, modified, must_build=False):
    trees, status = engine.upgma_batch(groups, kind=kind, modified=modified)
    _compare(oracle, groups, trees, status, kind, modified, must_build)


@pytest.fixture(scope="module")
def loaded(engine, oracle):
    seqs, where = _the_set(oracle)
    engine.upload_seqs(seqs)
    return engine, where


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_group_sizes(loaded, oracle, kind, modified):
    """Every size up to 1024 in one call (the 256-thread workgroup), then all of them with 1025 (the 1024-thread one)."""
    engine, where = loaded
    groups = [_size_group(where, m) for m in SIZES]
    _check(engine, oracle, groups[:-1], kind, modified)
    _check(engine, oracle, groups, kind, modified)


def _dense_group(where, m):
    return where["dense"][5:5 + m]


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_group_sizes_with_trees(loaded, oracle, kind, modified):
    """The same sizes cut from `dense`: every group has a tree, every record is compared."""
    engine, where = loaded
    groups = [_dense_group(where, m) for m in SIZES]
    _check(engine, oracle, groups[:-1], kind, modified, must_build=True)
    _check(engine, oracle, groups, kind, modified, must_build=True)


@pytest.mark.parametrize("modified", [False, True])
def test_the_cap(loaded, oracle, modified):
    engine, where = loaded
    assert len(where["n4096"]) == len(where["dense"]) == UPGMA_BATCH_MAX_MEMBERS
    _check(engine, oracle, [where["n4096"]], 1, modified)
    _check(engine, oracle, [where["dense"]], 1, modified, must_build=True)


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_named_groups_of_ties(loaded, oracle, kind, modified):
    """Id ties (ties), distance 0 (duplicates), prefixes of one sequence: equal keys and stale minima everywhere.
    duplicates and prefixes have trees; ties (600 sequences of 3 to 11 residues over three letters) holds pairs without a
    common residue and ends, in the reference as here, without a finite nearest neighbour."""
    engine, where = loaded
    _check(engine, oracle, [where[name] for name in TREES], kind, modified)
    _check(engine, oracle, [where["duplicates"], where["prefixes"]], kind, modified, must_build=True)


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_named_groups_with_lcs_zero(loaded, oracle, kind, modified):
    """Every distance the huge one (zero_only), LCS 0 at positive lengths (allx), scattered empty sequences: the status is
    `not ok` of the reference, whatever that is, and where a tree exists it is the reference's."""
    engine, where = loaded
    _check(engine, oracle, [where[name] for name in MAYBE], kind, modified)
    assert not _want(oracle, where["zero_only"], kind, modified)[2]


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_hub_group(loaded, oracle, kind, modified):
    engine, where = loaded
    assert len(where["hub"]) == 300
    _check(engine, oracle, [where["hub"]], kind, modified, must_build=True)


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_orientation_sensitive_group(loaded, oracle, kind, modified):
    """The quirk sequences are served without a flag: the triangle's orientation (ref = the later member) is
    UPGMA::computeDistances's.  Forwards, backwards (the other orientation of every pair) and among ordinary groups; the
    two orders see different distances wherever the oracle's square is asymmetric."""
    engine, where = loaded
    q = where["quirk"]
    back = q[::-1].copy()
    forwards, backwards = _distances(oracle, q, kind), _distances(oracle, back, kind)
    assert (_LCS[q.tobytes()] != _LCS[q.tobytes()].T).any()  # the set is what it is here for
    off = ~np.eye(len(q), dtype=bool)
    assert (forwards[off] != backwards[::-1, ::-1][off]).any()
    _check(engine, oracle, [q, where["dense"][:70], back], kind, modified, must_build=True)


def test_everything_in_one_call(loaded, oracle):
    """The named groups, the hub, the quirk group, the sizes and the cap in one call, an empty and a one-member group
    between them."""
    engine, where = loaded
    groups = []
    for ids in [where[name] for name in TREES + MAYBE + ["hub", "quirk"]] + [_size_group(where, m) for m in SIZES] + \
            [_dense_group(where, m) for m in SIZES] + [where["n4096"]]:
        groups += [ids, np.zeros(0, np.int32), where["ties"][5:6]]
    _check(engine, oracle, groups, 1, False)


def test_permuted_and_repeated_groups(loaded, oracle):
    """An id list that is neither contiguous nor ascending; the same list twice in one call (and a member twice in a list)."""
    engine, where = loaded
    rng = np.random.Generator(np.random.PCG64(5))
    everything = np.concatenate([where[name] for name in TREES] + [where["dense"][:600]])
    scattered = rng.permutation(everything)[:300].astype(np.int32)
    twice = where["duplicates"][:40]
    doubled = np.concatenate([where["prefixes"][:30], where["prefixes"][:30][::-1]]).astype(np.int32)
    for kind, modified in ((1, False), (0, True)):
        _check(engine, oracle, [scattered, twice, scattered[::-1].copy(), twice, doubled], kind, modified)
        assert _want(oracle, twice, kind, modified)[2] and _want(oracle, doubled, kind, modified)[2]


def test_a_good_group_next_to_one_without_a_tree(loaded, oracle):
    engine, where = loaded
    groups = [where["dense"][:50], where["zero_only"][:20], where["prefixes"][:40]]
    trees, status = engine.upgma_batch(groups, kind=1)  # (returns: the call is OK)
    assert list(status) == [0, 1, 0]
    _compare(oracle, groups, trees, status, 1, False)


def _outputs(groups):
    total = sum(max(len(g) - 1, 0) for g in groups)
    return np.full(total + 4, -7, np.int32), np.full(total + 4, -9, np.int32), np.full(len(groups) + 4, -11, np.int32)


def _are_untouched(out):
    return (out[0] == -7).all() and (out[1] == -9).all() and (out[2] == -11).all()


def test_refusals_leave_the_outputs_alone(loaded):
    engine, where = loaded
    too_many = np.concatenate([where["n4096"], where["ties"][:1]])
    assert len(too_many) == UPGMA_BATCH_MAX_MEMBERS + 1
    for groups, kind, pattern in (([where["ties"][:10], too_many], 1, r"lcsgpu error -6: .*4097 members"),
                                  ([where["ties"][:10], where["ties"][:20]], 7, r"lcsgpu error -1: .*unknown distance kind")):
        out = _outputs(groups)
        with pytest.raises(famsa_amd.LcsGpuError, match=pattern):
            engine.upgma_batch(groups, kind=kind, out=out)
        assert _are_untouched(out)
    # a group table that does not start at 0: the library's entry point itself
    ids = np.ascontiguousarray(where["ties"][:30], np.int32)
    offs = np.array([1, 10, 30], np.int64)
    out = _outputs([ids[:10], ids[10:]])
    rc = engine._lib.lcsgpu_upgma_batch(engine._ctx, ids.ctypes.data_as(C.POINTER(C.c_int32)), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                        2, 1, 0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    assert rc == -1 and b"group_offsets[0]" in engine._lib.lcsgpu_last_error()
    assert _are_untouched(out)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import famsa_amd, oracle_bind, test_gpu_upgma_batch as t
seqs, where = t._the_set(oracle_bind.Oracle())
eng = famsa_amd.LcsGpu(0)
eng.upload_seqs(seqs)
groups = t._sliced_groups(where)
for kind, modified in t.SLICED:
    trees, status = eng.upgma_batch(groups, kind=kind, modified=modified)
    np.save(sys.argv[2] + "/left_%d_%d.npy" % (kind, modified), np.concatenate([l for l, r in trees]))
    np.save(sys.argv[2] + "/right_%d_%d.npy" % (kind, modified), np.concatenate([r for l, r in trees]))
    np.save(sys.argv[2] + "/status_%d_%d.npy" % (kind, modified), status)
eng.close()
"""
SLICED = [(1, 0), (0, 1)]


def _sliced_groups(where):
    """3.1 MB of squares: with upgma_group_mb=1 the 600- and the 513-member group are each larger than a slice (a slice
    always holds one group) and the others share a third."""
    return [_size_group(where, 3), _size_group(where, 65), _dense_group(where, 257), _dense_group(where, 513), where["ties"],
            where["duplicates"][:300], where["zero_only"][:40]]


def test_many_slices_give_the_same_records(oracle, tmp_path):
    """LCSGPU_TUNE upgma_group_mb is read once per process: a child of its own cuts the groups into slices of 1 MB of
    squares (several launch pairs that reuse one square buffer)."""
    env = dict(os.environ)
    env["LCSGPU_TUNE"] = "upgma_group_mb=1"
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    _, where = _the_set(oracle)
    groups = _sliced_groups(where)
    for kind, modified in SLICED:
        left, right, status = (np.load(str(tmp_path / ("%s_%d_%d.npy" % (what, kind, modified)))) for what in ("left", "right", "status"))
        at, trees = 0, []
        for ids in groups:
            k = max(len(ids) - 1, 0)
            trees.append((left[at:at + k], right[at:at + k]))
            at += k
        assert at == len(left) == len(right)
        _compare(oracle, groups, trees, status, kind, bool(modified))
