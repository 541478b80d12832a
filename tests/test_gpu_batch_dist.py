"""Batch mode for distance matrices end to end: famsa_amd.dist_exports, `famsa-gpu -dist_export -batch <list>` and the C-ABI
call underneath (lcsgpu_dist_text_batch) -- every output equal to the reference-made golden where tests/golden has one, and
byte-equal to what the one-file call (famsa_amd.dist_export, resp. LcsGpu.dist_text of the list uploaded alone) gives
everywhere else.  tests/test_gpu_dist_text.py pins that one-file path to the reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import famsa_amd
import mst_shapes
from famsa_amd import lcsgpu, seqio
from famsa_amd.hostlib import CLI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
# (distance, square_matrix, pid)
MODES = [(d, sq, pid) for d in ("indel075_div_lcs", "indel_div_lcs") for sq in (False, True) for pid in (False, True)]
_ONE = {}


def _gold(rel):
    return open(os.path.join(G, rel), "rb").read()


def _one_file(path, mode, tmp):
    """famsa_amd.dist_export of one file, made once per (file, mode)."""
    key = (path, mode)
    if key not in _ONE:
        out = os.path.join(tmp, "one_%d.csv" % len(_ONE))
        famsa_amd.dist_export(path, out, distance=mode[0], square_matrix=mode[1], pid=mode[2])
        _ONE[key] = open(out, "rb").read()
        os.remove(out)
    return _ONE[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("batch_dist"))


@pytest.fixture(scope="module")
def zero_last(tmp):
    path = os.path.join(tmp, "zero_last.fasta")
    mst_shapes.write_zero_last_fasta(path)
    return path


def _short_fasta(path, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs = [rng.integers(0, 20, size=int(l)).astype(np.uint8) for l in rng.integers(8, 31, size=n)]
    codes, offsets = seqio.pack(seqs)
    seqio.to_fasta(codes, offsets, path, prefix="short")
    return path


def _batch(paths, mode, tmp, tag, **kw):
    outs = [os.path.join(tmp, "%s_%02d.csv" % (tag, k)) for k in range(len(paths))]
    res = famsa_amd.dist_exports(paths, outs, distance=mode[0], square_matrix=mode[1], pid=mode[2], **kw)
    return res, outs


# ---- 1. the reference's goldens through the batch ----

@pytest.mark.parametrize("name,square,pid", [("dist", False, False), ("pid", False, True), ("dist_sq", True, False), ("pid_sq", True, True)])
def test_reference_goldens_through_the_batch(tmp, name, square, pid):
    rels = ["adeno_fiber/adeno_fiber", "adversarial.fasta", "dummy/one-seq", "dummy/two-seq", "dummy/many-seq"]
    paths = [os.path.join(G, r) for r in rels]
    mode = ("indel075_div_lcs", square, pid)
    res, outs = _batch(paths, mode, tmp, "gold_" + name)
    assert res == [None] * len(paths)
    assert open(outs[0], "rb").read() == _gold("adeno_fiber/%s.csv" % name)
    if name == "dist_sq":  # carry-quirk refs and LCS 0 values: a square mirrored from a triangle fails here
        assert open(outs[1], "rb").read() == _gold("adversarial_dist_sq.csv")
        assert b"9223372036854775808.223372036854775808" in open(outs[1], "rb").read()
    if name == "pid":
        assert open(outs[1], "rb").read() == _gold("adversarial_pid.csv")
    for path, out in zip(paths[1:], outs[1:]):
        assert open(out, "rb").read() == _one_file(path, mode, tmp), path


# ---- 2. byte-equal to the one-file call ----

def _case2_paths(zero_last):
    return [os.path.join(G, "adeno_fiber_duplicates", "adeno_fiber_duplicates"), os.path.join(G, "adeno_fiber_extra", "adeno_fiber_extra"),
            os.path.join(G, "adversarial_long.fasta"), os.path.join(G, "adversarial_tree.fasta"), zero_last]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "%s%s%s" % (m[0], "-sq" if m[1] else "", "-pid" if m[2] else ""))
def test_byte_equal_to_the_one_file_call(tmp, zero_last, mode):
    paths = _case2_paths(zero_last)
    paths.append(paths[1])  # one file named twice in one list
    res, outs = _batch(paths, mode, tmp, "eq")
    assert res == [None] * len(paths)
    bad = [p for p, out in zip(paths, outs) if open(out, "rb").read() != _one_file(p, mode, tmp)]
    assert not bad, (mode, bad)


# ---- 3 .. 5, 7: the command line ----

def _write_list(tmp_path, paths, suffix):
    outs = [str(tmp_path / ("%02d_%s.csv" % (k, suffix))) for k in range(len(paths))]
    lst = str(tmp_path / ("list_%s.txt" % suffix))
    with open(lst, "w") as f:
        f.write("# input<TAB>output\n\n")
        for a, b in zip(paths, outs):
            f.write("%s\t%s\n" % (a, b))
    return lst, outs


def _run(args, host_test=None):
    env = dict(os.environ)
    env.pop("FAMSA_HOST_TEST", None)
    if host_test:
        env["FAMSA_HOST_TEST"] = host_test
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)


def _totals(stderr):
    return {k: v for k, v in re.findall(r"^(batch\.\w+|time\.\w+)=(\S+)$", stderr, re.M)}


MODE_FLAGS = {False: [], True: ["-square_matrix"]}


@pytest.mark.parametrize("square", [False, True])
def test_several_chunks_reuse_the_text_buffers(tmp, tmp_path, zero_last, square):
    """Nine files, a budget that gives the large ones a chunk each: the third chunk's text comes in the first one's buffer."""
    paths = _case2_paths(zero_last) + [os.path.join(G, r) for r in ("adeno_fiber/adeno_fiber", "dummy/one-seq", "dummy/two-seq", "dummy/many-seq")]
    lst, outs = _write_list(tmp_path, paths, "chunks")
    p = _run(["-dist_export", *MODE_FLAGS[square], "-batch", lst, "-v"], host_test="batch_pairs=30000")
    assert p.returncode == 0, p.stderr[-2000:]
    t = _totals(p.stderr)
    assert int(t["batch.files"]) == 9 and int(t["batch.chunks"]) >= 3 and int(t["batch.files_failed"]) == 0, t
    assert int(t["batch.files_in_chunks"]) + int(t["batch.files_one_file_route"]) == 9, t
    mode = ("indel075_div_lcs", square, False)
    total = 0
    for path, out in zip(paths, outs):
        got = open(out, "rb").read()
        assert got == _one_file(path, mode, tmp), path
        total += len(got) - (got.index(b"\n") + 1 if square else 0)
    if int(t["batch.files_one_file_route"]) == 0:
        assert int(t["batch.text_bytes"]) == total, t
    assert "time.store" in t and "time.load" in t and "time.gpu_upload" in t and "time.device" in t


def test_routing_by_the_record_count(tmp, tmp_path):
    paths = [os.path.join(G, r) for r in ("dummy/one-seq", "adeno_fiber/adeno_fiber", "dummy/two-seq", "dummy/many-seq")]
    lst, outs = _write_list(tmp_path, paths, "route")
    p = _run(["-dist_export", "-pid", "-batch", lst, "-v"], host_test="batch_group_max=100")
    assert p.returncode == 0, p.stderr[-2000:]
    t = _totals(p.stderr)
    assert int(t["batch.files_one_file_route"]) == 1 and int(t["batch.files_in_chunks"]) == 3 and int(t["batch.chunks"]) == 1, t
    assert open(outs[1], "rb").read() == _gold("adeno_fiber/pid.csv")
    mode = ("indel075_div_lcs", False, True)
    for path, out in zip(paths, outs):
        assert open(out, "rb").read() == _one_file(path, mode, tmp), path


def test_rows_of_several_segments(tmp, tmp_path):
    """1030 members: rows of 1023, 1024 and 1025 values sit on the seam between the first and the second segment; 2050
    members in the lower form: a third segment."""
    a = _short_fasta(os.path.join(tmp, "short1030.fasta"), 1030, 5)
    b = _short_fasta(os.path.join(tmp, "short2050.fasta"), 2050, 6)
    for square, paths in ((False, [a, b]), (True, [a])):
        lst, outs = _write_list(tmp_path, paths, "seg%d" % square)
        p = _run(["-dist_export", *MODE_FLAGS[square], "-batch", lst, "-v"], host_test="batch_group_max=4096")
        assert p.returncode == 0, p.stderr[-2000:]
        t = _totals(p.stderr)
        assert int(t["batch.files_in_chunks"]) == len(paths) and int(t["batch.files_one_file_route"]) == 0, t
        for path, out in zip(paths, outs):
            assert open(out, "rb").read() == _one_file(path, ("indel075_div_lcs", square, False), tmp), (path, square)


def test_a_file_that_fails_fails_alone(tmp, tmp_path):
    empty = str(tmp_path / "empty.fasta")
    open(empty, "w").close()
    good = [os.path.join(G, r) for r in ("adeno_fiber/adeno_fiber", "dummy/many-seq", "dummy/two-seq")]
    paths = [good[0], str(tmp_path / "missing.fasta"), good[1], empty, good[2], good[1]]
    lst, outs = _write_list(tmp_path, paths, "fail")
    outs[5] = str(tmp_path / "no_such_directory" / "out.csv")
    with open(lst, "w") as f:
        for a, b in zip(paths, outs):
            f.write("%s\t%s\n" % (a, b))
    p = _run(["-dist_export", "-batch", lst, "-v"])
    assert p.returncode == 2, p.stderr[-2000:]
    errors = [l for l in p.stderr.splitlines() if l.startswith("[ERROR]")]
    assert len(errors) == 3, p.stderr[-2000:]
    assert any(l.startswith("[ERROR] %s: " % paths[1]) for l in errors)
    assert any(l.startswith("[ERROR] %s: " % empty) and "no sequences in" in l for l in errors)
    assert any(l.startswith("[ERROR] %s: " % paths[5]) and "cannot open" in l for l in errors)
    assert int(_totals(p.stderr)["batch.files_failed"]) == 3
    mode = ("indel075_div_lcs", False, False)
    for k in (0, 2, 4):
        assert open(outs[k], "rb").read() == _one_file(paths[k], mode, tmp), paths[k]
    assert not os.path.exists(outs[1]) and not os.path.exists(outs[3])
    # the same list from Python
    outs2 = [o + ".py" for o in outs]
    res = famsa_amd.dist_exports(paths, outs2, on_error="return")
    assert [isinstance(r, Exception) for r in res] == [False, True, False, True, False, True], res
    assert all(r is None for r in res if not isinstance(r, Exception))
    for k in (0, 2, 4):
        assert open(outs2[k], "rb").read() == _one_file(paths[k], mode, tmp)
    with pytest.raises(RuntimeError):
        famsa_amd.dist_exports(paths, outs2)


# ---- 6. the C-ABI directly ----

@pytest.fixture(scope="module")
def small_set():
    """adversarial.fasta (carry-quirk refs, LCS 0 pairs) and a few adeno_fiber members, names without '>'."""
    ids, seqs = seqio.read_fasta(os.path.join(G, "adversarial.fasta"))
    ids2, seqs2 = seqio.read_fasta(os.path.join(G, "adeno_fiber", "adeno_fiber"))
    ids, seqs = ids + ids2[:20], seqs + seqs2[:20]
    return [i[1:] for i in ids], [lcsgpu.encode(s) for s in seqs]


def _lists(n):
    rng = np.random.Generator(np.random.PCG64(17))
    return [rng.permutation(n).tolist(),             # the whole set, permuted
            list(range(0, n, 3)),                     # not contiguous
            [],                                       # empty
            [n - 1],                                  # one member
            [5, 2, n - 1, 0, 9],                      # shares ids with the others, not in upload order
            list(range(n - 1, n // 2, -1)),           # descending
            [7, 3]]


def _alone(engine, names, enc, lists, **mode):
    """Every list uploaded alone in list order through the one-file calls."""
    want = []
    for ids in lists:
        if not ids:
            want.append(b"")
            continue
        engine.upload_seqs([enc[i] for i in ids])
        want.append(engine.dist_text([names[i] for i in ids], [(0, len(ids))], **mode))
    return want


@pytest.mark.parametrize("mode", [dict(kind=1), dict(kind=0), dict(kind=1, square=True), dict(kind=0, square=True), dict(pid=True),
                                  dict(pid=True, square=True)], ids=str)
def test_abi_lists_against_each_list_uploaded_alone(engine, small_set, mode):
    names, enc = small_set
    lists = _lists(len(enc))
    engine.upload_seqs(enc)
    got = engine.dist_text_batch(names, lists, **mode)
    assert got[2] == b"" and (mode.get("square") or got[3] == (names[lists[3][0]] + "\n").encode("latin-1"))
    assert got == _alone(engine, names, enc, lists, **mode)


def test_abi_a_call_without_any_pair(engine, small_set):
    names, enc = small_set
    engine.upload_seqs(enc)
    got = engine.dist_text_batch(names, [[4], [], [0], [4]])
    assert got == [(names[4] + "\n").encode("latin-1"), b"", (names[0] + "\n").encode("latin-1"), (names[4] + "\n").encode("latin-1")]
    assert engine.dist_text_batch(names, []) == [] and engine.dist_text_batch(names, [[], []]) == [b"", b""]


def test_abi_a_calls_text_outlives_the_next_call(engine, small_set):
    names, enc = small_set
    lists = _lists(len(enc))
    engine.upload_seqs(enc)
    first = engine.dist_text_batch(names, lists[:4], copy=False)   # views of the context's buffer
    second = engine.dist_text_batch(names, lists[4:], square=True, copy=False)
    first_after = [bytes(v) for v in first]                       # read AFTER the second call
    second_now = [bytes(v) for v in second]
    assert first_after == _alone(engine, names, enc, lists[:4])
    assert second_now == _alone(engine, names, enc, lists[4:], square=True)


def test_abi_refusals_leave_the_outputs_alone(engine, small_set):
    names, enc = small_set
    n = len(enc)
    engine.upload_seqs(enc)
    raw = [x.encode("latin-1") for x in names]
    name_off = np.zeros(n + 1, np.uint64)
    name_off[1:] = np.cumsum([len(x) for x in raw])
    blob = b"".join(raw)
    lib, ctx = engine._lib, engine._ctx

    def call(ids, offs, names_ptr=blob, off_ptr=None, text=True, text_off=True, ids_null=False):
        ids = np.ascontiguousarray(ids, np.int32)
        offs = np.ascontiguousarray(offs, np.int64)
        sentinel = np.full(len(offs), 0xABABABABABABABAB, np.uint64)
        ptr = C.c_void_p(0x1234)
        rc = lib.lcsgpu_dist_text_batch(ctx, names_ptr, name_off.ctypes.data if off_ptr is None else off_ptr, None if ids_null else ids.ctypes.data,
                                        offs.ctypes.data, len(offs) - 1, 1, 0, C.byref(ptr) if text else None,
                                        sentinel.ctypes.data if text_off else None)
        assert (sentinel == 0xABABABABABABABAB).all() and ptr.value == 0x1234
        return rc

    E_INVALID, E_UNSUPPORTED = -1, -6
    assert call(np.arange(4097) % n, [0, 4097]) == E_UNSUPPORTED
    assert call(np.arange(4099) % n, [0, 2, 4099]) == E_UNSUPPORTED  # (the list's size counts, not the ids it names)
    assert call([0, 1, n], [0, 3]) == E_INVALID and call([0, -1], [0, 2]) == E_INVALID
    assert call([0, 1, 2], [0, 3], text=False) == E_INVALID
    assert call([0, 1, 2], [0, 3], text_off=False) == E_INVALID
    assert call([0, 1, 2], [0, 3], off_ptr=0) == E_INVALID
    assert call([0, 1, 2], [0, 3], names_ptr=None) == E_INVALID
    assert call([0, 1, 2], [0, 3], ids_null=True) == E_INVALID
    assert call([0, 1, 2], [0, 3, 2]) == E_INVALID  # descending offsets
    # and the context still serves
    assert engine.dist_text_batch(names, [[1, 0]])[0].startswith(raw[1] + b"\n" + raw[0] + b",")
