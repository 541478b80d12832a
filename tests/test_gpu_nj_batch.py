"""lcsgpu_nj_batch -- neighbour joining of many id lists of one uploaded set, one workgroup per list -- against a reference
that is NOT the engine: NeighborJoining::computeTree in numpy float32 (nj_ref.nj_tree, pinned by test_nj_ref.py) over the
oracle's distances of the oracle's LCS values, list by list, in the list's own order and with the triangle's orientation
(ref = the later member).  One set is uploaded for the whole file: the set of test_gpu_upgma_batch.py (the degenerate sets
of mst_shapes.py, 4096 short random sequences, the orientation-sensitive sequences, a hub family of 300, 4096 random
sequences over four letters: `dense`).  left / right are compared exactly (tolerance 0); status must be `not ok` of the
helper.

A pair with LCS 0 has the distance FLT_MAX; two of them in a row make the row's sum +inf and its q NaN or -inf, and sooner
or later no q is below FLT_MAX: the fate of every size group cut from the 20-letter set from 63 members on and of ties,
allx, zero_only and zero_scattered (checked on the CPU with the helper; the tests assert it where they rely on it).  There
the status must say so; every size is therefore cut from `dense`, where every pair shares a residue and the helper builds
a tree.

Group sizes: 0 and 1 (no record), 2 (one record, no merge), 3, 4, 63 / 64 / 65 (a chunk of columns of the scan),
199 / 200 / 201 (around WIDE_AT, from which a list runs in 1024 threads), 255 / 256 / 257 (the stride of the 256-thread
workgroup), 1023 / 1024 / 1025 (the stride of the 1024-thread workgroup); all of them in one call, and again with
LCSGPU_TUNE nj_group_threads forcing each thread count on every size.  The cap, 2048 members, is compared with
engine.nj() of the same list uploaded alone (pinned to the reference at 4188 and 13 774 sequences by
test_gpu_endtoend.py / test_gpu_scale.py): the helper would take a minute there."""
import ctypes as C
import os

import numpy as np
import pytest

import famsa_amd
import nj_ref
import test_gpu_upgma_batch as upgma_batch
from famsa_amd.lcsgpu import NJ_BATCH_MAX_MEMBERS

pytestmark = pytest.mark.gpu
WIDE_AT = 200  # NJ_GROUP_WIDE_AT of famsa_amd/csrc/fasttree_kernels.h
SIZES = sorted({0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, WIDE_AT - 1, WIDE_AT, WIDE_AT + 1, 1023, 1024, 1025})
NO_TREE = ["ties", "zero_only", "allx", "zero_scattered"]
TREES = ["duplicates", "prefixes"]
_REF = {}
_the_set = upgma_batch._the_set
_distances = upgma_batch._distances
_size_group = upgma_batch._size_group
_dense_group = upgma_batch._dense_group
_outputs = upgma_batch._outputs
_are_untouched = upgma_batch._are_untouched


def _want(oracle, ids, kind):
    """The helper's (left, right, ok) of one id list: computed once per (list, kind), shared read-only."""
    key = (np.asarray(ids, np.int32).tobytes(), kind)
    if key not in _REF:
        if len(ids) < 2:
            want = (np.zeros(0, np.int32), np.zeros(0, np.int32), True)
        else:
            want = nj_ref.nj_tree(_distances(oracle, ids, kind))
        want[0].flags.writeable = False
        want[1].flags.writeable = False
        _REF[key] = want
    return _REF[key]


def _compare(oracle, groups, trees, status, kind, must_build=False):
    assert len(trees) == len(groups) and len(status) == len(groups)
    bad = []
    for g, (ids, (left, right)) in enumerate(zip(groups, trees)):
        wl, wr, ok = _want(oracle, ids, kind)
        if must_build and not ok:
            bad.append((g, len(ids), "the helper builds no tree here"))
        elif int(status[g]) != (0 if ok else 1):
            bad.append((g, len(ids), "status %d, helper ok = %s" % (status[g], ok)))
        elif ok and not (len(left) == len(wl) and (left == wl).all() and (right == wr).all()):
            k = int(np.flatnonzero((left != wl) | (right != wr))[0]) if len(left) == len(wl) else -1
            bad.append((g, len(ids), "node %d: got (%d, %d), want (%d, %d)" % (k, left[k], right[k], wl[k], wr[k]) if k >= 0
                        else "%d records, want %d" % (len(left), len(wl))))
    assert not bad, (kind, bad)


def _check(engine, oracle, groups, kind, must_build=False):
    trees, status = engine.nj_batch(groups, kind=kind)
    _compare(oracle, groups, trees, status, kind, must_build)


def _tune(monkeypatch, setting):
    """LCSGPU_TUNE nj_group_threads / nj_group_mb are read at every call: one process serves."""
    before = os.environ.get("LCSGPU_TUNE")
    monkeypatch.setenv("LCSGPU_TUNE", setting if not before else before + "," + setting)


@pytest.fixture(scope="module")
def loaded(engine, oracle):
    seqs, where = _the_set(oracle)
    engine.upload_seqs(seqs)
    return engine, where


@pytest.mark.parametrize("threads", [0, 256, 1024])
@pytest.mark.parametrize("kind", [1, 0])
def test_group_sizes(loaded, oracle, monkeypatch, kind, threads):
    """Every size cut from `dense` in one call: every group has a tree, every record is compared.  threads = 0: each
    size in the workgroup of its own choice (two launches of merges); 256 / 1024: all of them in that one."""
    engine, where = loaded
    if threads:
        _tune(monkeypatch, "nj_group_threads=%d" % threads)
    _check(engine, oracle, [_dense_group(where, m) for m in SIZES], kind, must_build=True)


@pytest.mark.parametrize("kind", [1, 0])
def test_the_small_sizes_alone(loaded, oracle, kind):
    """No list with a merge (0, 1, 2 members), then lists up to four members: the calls whose launches are the smallest."""
    engine, where = loaded
    _check(engine, oracle, [_dense_group(where, m) for m in (0, 1, 2)], kind, must_build=True)
    _check(engine, oracle, [_dense_group(where, m) for m in (0, 1)], kind, must_build=True)
    _check(engine, oracle, [_dense_group(where, m) for m in (3, 4, 2, 3)], kind, must_build=True)
    trees, status = engine.nj_batch([_dense_group(where, 2)], kind=kind)
    assert list(status) == [0] and trees[0][0].tolist() == [0] and trees[0][1].tolist() == [1]


@pytest.mark.parametrize("threads", [0, 256])
def test_the_cap(loaded, oracle, monkeypatch, threads):
    """2048 members against lcsgpu_nj of the same list uploaded alone, in the list's order."""
    engine, where = loaded
    seqs, _ = _the_set(oracle)
    ids = where["dense"][1000:1000 + NJ_BATCH_MAX_MEMBERS]
    assert len(ids) == NJ_BATCH_MAX_MEMBERS
    if "cap" not in _REF:
        try:
            engine.upload_seqs([seqs[i] for i in ids])
            left, right = engine.nj(kind=1)
            _REF["cap"] = (left.copy(), right.copy())
        finally:
            engine.upload_seqs(seqs)
    if threads:
        _tune(monkeypatch, "nj_group_threads=%d" % threads)
    trees, status = engine.nj_batch([ids, _dense_group(where, 70)], kind=1)
    assert list(status) == [0, 0]
    assert (trees[0][0] == _REF["cap"][0]).all() and (trees[0][1] == _REF["cap"][1]).all()
    _compare(oracle, [_dense_group(where, 70)], trees[1:], status[1:], 1, must_build=True)


@pytest.mark.parametrize("kind", [1, 0])
def test_hub_group(loaded, oracle, kind):
    """One row re-created merge after merge."""
    engine, where = loaded
    assert len(where["hub"]) == 300
    _check(engine, oracle, [where["hub"]], kind, must_build=True)


@pytest.mark.parametrize("kind", [1, 0])
def test_groups_of_the_twenty_letter_set_and_the_degenerate_shapes(loaded, oracle, kind):
    """The status is `not ok` of the helper, whatever that is; where a tree exists it is the helper's."""
    engine, where = loaded
    groups = [_size_group(where, m) for m in upgma_batch.SIZES] + [where[name] for name in NO_TREE + TREES]
    _check(engine, oracle, groups, kind)
    for name in NO_TREE:
        assert not _want(oracle, where[name], kind)[2], name
    _check(engine, oracle, [where[name] for name in TREES], kind, must_build=True)


def test_a_good_group_next_to_groups_without_a_tree(loaded, oracle):
    engine, where = loaded
    groups = [_dense_group(where, 50), where["zero_only"][:20], where["prefixes"][:40], where["allx"], _dense_group(where, 300)]
    trees, status = engine.nj_batch(groups, kind=1)  # (returns: the call is OK)
    assert list(status) == [0, 1, 0, 1, 0]
    _compare(oracle, groups, trees, status, 1)


@pytest.mark.parametrize("kind", [1, 0])
def test_orientation_sensitive_group(loaded, oracle, kind):
    """The quirk sequences are served without a flag: forwards and backwards (the other orientation of every pair)."""
    engine, where = loaded
    q = where["quirk"]
    _check(engine, oracle, [q, _dense_group(where, 70), q[::-1].copy()], kind, must_build=True)


def test_permuted_and_repeated_groups(loaded, oracle):
    """The same ids in two lists (and a member twice in a list); lists in descending and in shuffled id order."""
    engine, where = loaded
    rng = np.random.Generator(np.random.PCG64(5))
    dense = where["dense"][:600]
    shuffled = rng.permutation(dense)[:300].astype(np.int32)
    twice = where["duplicates"][:40]
    doubled = np.concatenate([where["prefixes"][:30], where["prefixes"][:30][::-1]]).astype(np.int32)
    for kind in (1, 0):
        _check(engine, oracle, [shuffled, twice, dense[:257][::-1].copy(), twice, shuffled[::-1].copy(), doubled, dense[:257]], kind)
        assert _want(oracle, shuffled, kind)[2] and _want(oracle, dense[:257][::-1].copy(), kind)[2]


def test_every_list_a_slice_of_its_own(loaded, oracle, monkeypatch):
    """nj_group_mb=1 (the smallest slice there is: 262144 floats).  First four lists of 513 to 725 members, 131328 floats
    at the least: no two fit one slice, so every list is a slice of its own and four launch pairs reuse one float buffer.
    Then a mixed call, whose lists sort into the slices [725], [600] and [513, 300, 257, 65, 40, 3]: a slice of several
    jobs behind slices of one, with jobs on both sides of the thread-count switch."""
    engine, where = loaded
    _tune(monkeypatch, "nj_group_mb=1")
    alone = [_dense_group(where, 513), _dense_group(where, 725), where["dense"][2000:2600], _dense_group(where, 600)]
    assert all(2 * (len(g) * (len(g) - 1) // 2) > (1 << 20) // 4 for g in alone)
    _check(engine, oracle, alone, 1, must_build=True)
    groups = [_dense_group(where, 3), _dense_group(where, 65), _dense_group(where, 725), where["zero_only"][:40], _dense_group(where, 513),
              where["hub"], _dense_group(where, 600), _dense_group(where, 257)]
    for kind in (1, 0):
        _check(engine, oracle, groups, kind)
        assert [_want(oracle, g, kind)[2] for g in groups] == [True, True, True, False, True, True, True, True]


def test_refusals_leave_the_outputs_alone(loaded):
    engine, where = loaded
    too_many = where["dense"][:NJ_BATCH_MAX_MEMBERS + 1]
    assert len(too_many) == NJ_BATCH_MAX_MEMBERS + 1
    out_of_range = np.array([0, 1, len(_the_set(None)[0])], np.int32)
    for groups, kind, pattern in (([where["dense"][:10], too_many], 1, r"lcsgpu error -6: .*2049 members"),
                                  ([where["dense"][:10], where["dense"][:20]], 7, r"lcsgpu error -1: .*unknown distance kind"),
                                  ([where["dense"][:10], out_of_range], 1, r"lcsgpu error -1: .*out of range"),
                                  ([where["dense"][:10], np.array([3, -1], np.int32)], 0, r"lcsgpu error -1: .*out of range")):
        out = _outputs(groups)
        with pytest.raises(famsa_amd.LcsGpuError, match=pattern):
            engine.nj_batch(groups, kind=kind, out=out)
        assert _are_untouched(out)
    # NULL outputs, and a group table that does not start at 0: the library's entry point itself
    ids = np.ascontiguousarray(where["dense"][:30], np.int32)
    pi, po = ids.ctypes.data_as(C.POINTER(C.c_int32)), C.POINTER(C.c_int64)
    offs = np.array([0, 10, 30], np.int64)
    out = _outputs([ids[:10], ids[10:]])
    call = engine._lib.lcsgpu_nj_batch
    for left, right, status in ((None, out[1].ctypes.data, out[2].ctypes.data), (out[0].ctypes.data, None, out[2].ctypes.data),
                                (out[0].ctypes.data, out[1].ctypes.data, None)):
        assert call(engine._ctx, pi, offs.ctypes.data_as(po), 2, 1, left, right, status) == -1
        assert b"NULL out" in engine._lib.lcsgpu_last_error()
        assert _are_untouched(out)
    offs = np.array([1, 10, 30], np.int64)
    assert call(engine._ctx, pi, offs.ctypes.data_as(po), 2, 1, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data) == -1
    assert b"group_offsets[0]" in engine._lib.lcsgpu_last_error()
    assert _are_untouched(out)
    # and the engine still serves
    trees, status = engine.nj_batch([ids[:2]], kind=1)
    assert list(status) == [0] and trees[0][0].tolist() == [0]
