"""lcsgpu_mst_prim_batch -- Prim's MST of many id lists of one uploaded set, one workgroup per list -- against a reference
that is NOT the engine: MSTPrim's recurrence in numpy (mst_ref.prim_edges_fast) over distances made from the oracle's LCS
values (mst_ref.DistanceRows), list by list, in the list's own order and with the triangle's orientation (ref = the later
member).  One set is uploaded for the whole file: the degenerate sets of mst_shapes.py laid end to end, 4096 short random
sequences (lengths 5-40: the oracle's triangle of the largest group stays small) and the orientation-sensitive sequences of
tests/golden/adversarial_tree.fasta.

Group sizes: 0 and 1 (no record), 2 and 3 (the smallest that yield records), 63 / 64 / 65 (a wave), 255 / 256 / 257 (the
stride of the 256-thread workgroup), 1023 / 1024 / 1025 (the stride of the 1024-thread workgroup, and the size from which a
launch uses it), 4096 (the cap).  Records are compared exactly: from, to and the bits of dist."""
import os
import subprocess
import sys

import numpy as np
import pytest

import famsa_amd
import mst_ref
import mst_shapes
from famsa_amd import seqio
from famsa_amd.lcsgpu import MST_BATCH_MAX_MEMBERS, MST_EDGE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NAMED = ["zero_only", "ties", "duplicates", "allx", "zero_scattered", "prefixes"]
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
_SET = {}
_REF = {}
_SQ = {}


def _same(a, b):
    return len(a) == len(b) and (a["from"] == b["from"]).all() and (a["to"] == b["to"]).all() and \
        (a["dist"].view(np.uint64) == b["dist"].view(np.uint64)).all()


def _first_difference(got, want):
    if len(got) != len(want):
        return "%d records, want %d" % (len(got), len(want))
    for k in range(len(want)):
        if tuple(got[k]) != tuple(want[k]) or got["dist"][k:k + 1].view(np.uint64) != want["dist"][k:k + 1].view(np.uint64):
            return "edge %d: got %s, want %s" % (k, got[k], want[k])
    return "no difference"


def _the_set(oracle):
    """(sequences, {name: id range}) -- built once."""
    if not _SET:
        seqs, where = [], {}
        for name in NAMED + ["n4096"]:
            part = mst_shapes.build(name)
            where[name] = np.arange(len(seqs), len(seqs) + len(part), dtype=np.int32)
            seqs += part
        _, residues = seqio.read_fasta(os.path.join(G, "adversarial_tree.fasta"))
        part = [oracle.encode(r) for r in residues]
        where["quirk"] = np.arange(len(seqs), len(seqs) + len(part), dtype=np.int32)
        seqs += part
        _SET["seqs"], _SET["where"] = seqs, where
        _SET["packed"] = seqio.pack(seqs)
        _SET["lens"] = np.array([len(s) for s in seqs], np.int64)
    return _SET["seqs"], _SET["where"]


def _want(oracle, ids, kind):
    """The reference's records of one id list: computed once per (list, kind), shared read-only."""
    key = (np.asarray(ids, np.int32).tobytes(), kind)
    if key not in _REF:
        ids = np.asarray(ids, np.int32)
        m = len(ids)
        if m < 2:
            want = np.zeros(0, MST_EDGE)
        else:
            if key[0] not in _SQ:  # (both kinds share the LCS values)
                codes, offsets = _SET["packed"]
                _SQ[key[0]] = mst_ref.square_lcs(oracle.rect(codes, offsets, ids, ids), m)  # rect[k, c] = LCS(ref = list[k], partner = list[c])
            rows = mst_ref.DistanceRows(_SQ[key[0]], _SET["lens"][ids], kind, oracle)  # (the lower triangle: ref = the later member)
            want = mst_ref.prim_edges_fast(rows)
        want.flags.writeable = False
        _REF[key] = want
    return _REF[key]


def _size_group(where, m):
    """m members: an odd start inside the 4096 random sequences, every third of it from the `ties` set (id tie-breaks)."""
    ids = where["n4096"][7:7 + m].copy()
    ids[::3] = where["ties"][: len(ids[::3])]
    return ids


def _check(engine, oracle, groups, kind, flag):
    got = engine.mst_prim_batch(groups, kind=kind, triangle_orientation=flag)
    assert len(got) == len(groups)
    bad = []
    for g, ids in zip(got, groups):
        want = _want(oracle, ids, kind)
        if not _same(g, want):
            bad.append((len(ids), _first_difference(g, want)))
    assert not bad, (kind, flag, bad)


@pytest.fixture(scope="module")
def loaded(engine, oracle):
    seqs, where = _the_set(oracle)
    engine.upload_seqs(seqs)
    flags = engine.orientation_flags()
    assert flags[where["quirk"]].sum() > 0 and flags.sum() == flags[where["quirk"]].sum()
    return engine, where


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_group_sizes(loaded, oracle, kind, flag):
    """Every size up to 1024 in one call (the 256-thread workgroup), then all of them with 1025 (the 1024-thread one)."""
    engine, where = loaded
    groups = [_size_group(where, m) for m in SIZES]
    _check(engine, oracle, groups[:-1], kind, flag)
    _check(engine, oracle, groups, kind, flag)


@pytest.mark.parametrize("kind", [1, 0])
def test_the_cap(loaded, oracle, kind):
    engine, where = loaded
    assert len(where["n4096"]) == MST_BATCH_MAX_MEMBERS
    _check(engine, oracle, [where["n4096"]], kind, False)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("kind", [1, 0])
def test_named_groups(loaded, oracle, kind, flag):
    """Every distance the huge one (zero_only), id tie-breaks (ties), distance 0 (duplicates), LCS 0 at positive lengths
    (allx), scattered empty sequences, prefixes of one sequence."""
    engine, where = loaded
    _check(engine, oracle, [where[name] for name in NAMED], kind, flag)


def test_everything_in_one_call(loaded, oracle):
    """The named groups, the sizes and the cap in one call, an empty and a one-member group between them."""
    engine, where = loaded
    groups = []
    for ids in [where[name] for name in NAMED] + [_size_group(where, m) for m in SIZES] + [where["n4096"]]:
        groups += [ids, np.zeros(0, np.int32), where["ties"][5:6]]
    _check(engine, oracle, groups, 1, False)


def test_permuted_and_repeated_groups(loaded, oracle):
    """An id list that is neither contiguous nor ascending; the same list twice in one call (and a member twice in a list)."""
    engine, where = loaded
    rng = np.random.Generator(np.random.PCG64(5))
    everything = np.concatenate([where[name] for name in NAMED])
    scattered = rng.permutation(everything)[:300].astype(np.int32)
    twice = where["duplicates"][:40]
    doubled = np.concatenate([where["prefixes"][:30], where["prefixes"][:30][::-1]]).astype(np.int32)
    for kind in (1, 0):
        _check(engine, oracle, [scattered, twice, scattered[::-1].copy(), twice, doubled], kind, False)


def _untouched(engine, groups, kind, flag, pattern):
    total = sum(max(len(g) - 1, 0) for g in groups)
    out = np.zeros(total + 4, MST_EDGE)
    out["from"], out["to"], out["dist"] = -7, -9, 12345.5
    with pytest.raises(famsa_amd.LcsGpuError, match=pattern):
        engine.mst_prim_batch(groups, kind=kind, triangle_orientation=flag, out=out)
    assert (out["from"] == -7).all() and (out["to"] == -9).all() and (out["dist"] == 12345.5).all()


def test_refusals_leave_the_output_alone(loaded):
    engine, where = loaded
    too_many = np.concatenate([where["n4096"], where["ties"][:1]])
    assert len(too_many) == MST_BATCH_MAX_MEMBERS + 1
    _untouched(engine, [where["ties"][:10], too_many], 1, False, r"lcsgpu error -6: .*4097 members")
    _untouched(engine, [where["ties"][:10], too_many], 1, True, r"lcsgpu error -6: .*4097 members")
    _untouched(engine, [where["ties"][:10], where["quirk"]], 1, False, r"lcsgpu error -6: .*orientation sensitive")
    _untouched(engine, [where["ties"][:10], where["quirk"]], 0, False, r"lcsgpu error -6: .*orientation sensitive")


@pytest.mark.parametrize("kind", [1, 0])
def test_orientation_sensitive_group_with_the_flag(loaded, oracle, kind):
    """With LCSGPU_MST_TRIANGLE_ORIENTATION the quirk sequences are served: the reference over the LCS values of the
    triangle's orientation (ref = the later member) -- forwards, backwards (the other orientation of every pair) and among
    ordinary groups."""
    engine, where = loaded
    q = where["quirk"]
    codes, offsets = _SET["packed"]
    sq = oracle.rect(codes, offsets, q, q)
    assert (sq != sq.T).any()  # the set is what it is here for
    _check(engine, oracle, [q, where["ties"][:70], q[::-1].copy()], kind, True)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import famsa_amd, oracle_bind, test_gpu_mst_batch as t
seqs, where = t._the_set(oracle_bind.Oracle())
eng = famsa_amd.LcsGpu(0)
eng.upload_seqs(seqs)
groups = t._other_layout_groups(where)
for kind in (1, 0):
    got = eng.mst_prim_batch(groups, kind=kind)
    np.save(sys.argv[2] + "/edges_%d.npy" % kind, np.concatenate(got))
eng.close()
"""


def _other_layout_groups(where):
    return [_size_group(where, m) for m in (3, 65, 257, 1025)] + [where["ties"], where["duplicates"], where["zero_only"]]


def test_the_other_way_to_read_the_triangle(oracle, tmp_path):
    """LCSGPU_TUNE mst_batch_square is read once per process: a child of its own runs the setting that is not the default
    (the packed triangle read as it is) on sizes around every stride and three of the named groups."""
    env = dict(os.environ)
    env["LCSGPU_TUNE"] = "mst_batch_square=0"
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    _, where = _the_set(oracle)
    groups = _other_layout_groups(where)
    for kind in (1, 0):
        flat = np.load(str(tmp_path / ("edges_%d.npy" % kind)))
        at, bad = 0, []
        for ids in groups:
            want = _want(oracle, ids, kind)
            got = flat[at:at + len(want)]
            at += len(want)
            if not _same(got, want):
                bad.append((len(ids), _first_difference(got, want)))
        assert at == len(flat) and not bad, (kind, bad)
