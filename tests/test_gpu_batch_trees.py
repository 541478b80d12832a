"""Batch mode end to end: famsa_amd.guide_trees and `famsa-gpu -gt_export -batch <list>` over real families, degenerate
files and files that fail -- every output equal to the reference-made golden where tests/golden has one, and byte-equal
to what the one-file call gives for the same file everywhere else.  Where the one-file call refuses a file -- UPGMA and
NJ are undefined when no pair of the set has a finite distance left, which the block of empty sequences of zero_last
brings about ("no finite nearest neighbour", "no finite q") -- the batch must fail that file, and only that file, for
the same reason."""
import os
import re
import subprocess

import pytest

import famsa_amd
import mst_shapes
from famsa_amd.hostlib import CLI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
GTS = ["sl", "slink", "upgma", "nj"]
FILES = ["adeno_fiber/adeno_fiber", "adeno_fiber_duplicates/adeno_fiber_duplicates", "adeno_fiber_extra/adeno_fiber_extra",
         "hemopexin/hemopexin", "dummy/one-seq", "dummy/two-seq", "dummy/many-seq", "adversarial_tree.fasta"]
GOLD = {"adeno_fiber/adeno_fiber": {gt: "adeno_fiber/%s.dnd" % gt for gt in GTS},
        "hemopexin/hemopexin": {gt: "hemopexin/%s.dnd" % gt for gt in GTS},
        "adeno_fiber_duplicates/adeno_fiber_duplicates": {"sl": "adeno_fiber_duplicates/sl.dnd"},
        "adversarial_tree.fasta": {gt: "adversarial_tree_%s.dnd" % gt for gt in GTS}}
_ONE = {}


def _gold(rel):
    return open(os.path.join(G, rel), "rb").read()


def _one_file(path, gt, **kw):
    """famsa_amd.guide_tree of one file -- its text, or the RuntimeError it raises -- made once per (file, options)."""
    key = (path, gt, tuple(sorted(kw.items())))
    if key not in _ONE:
        try:
            _ONE[key] = famsa_amd.guide_tree(path, gt=gt, **kw)
        except RuntimeError as e:
            _ONE[key] = e
    return _ONE[key]


def _agree(got, want):
    """Equal texts, or both a failure for the same reason."""
    if isinstance(want, Exception):
        return isinstance(got, Exception) and "no finite" in str(want) and "no finite" in str(got)
    return got == want


@pytest.fixture(scope="module")
def zero_last(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("batch") / "zero_last.fasta")
    mst_shapes.write_zero_last_fasta(path)
    return path


def _want(path, rel, gt, **kw):
    return _gold(GOLD[rel][gt]) if gt in GOLD.get(rel, {}) else _one_file(path, gt, **kw)


@pytest.mark.parametrize("gt", GTS)
def test_guide_trees_against_goldens_and_the_one_file_call(zero_last, gt):
    paths = [os.path.join(G, rel) for rel in FILES] + [zero_last]
    got = famsa_amd.guide_trees(paths, gt=gt, on_error="return")
    assert len(got) == len(paths)
    bad = [rel for rel, path, text in zip(FILES + ["zero_last"], paths, got) if not _agree(text, _want(path, rel, gt))]
    assert not bad, (gt, bad)
    assert not any(isinstance(text, Exception) for text in got[:-1])  # only zero_last may be refused, and only as the one-file call refuses it
    assert got[FILES.index("dummy/one-seq")] == b""  # one sequence: no tree (the reference skips the stage)


@pytest.mark.parametrize("gt", GTS)
def test_keep_duplicates(zero_last, gt):
    dup = os.path.join(G, "adeno_fiber_duplicates", "adeno_fiber_duplicates")
    got = famsa_amd.guide_trees([dup, zero_last, dup], gt=gt, keep_duplicates=True, on_error="return")
    assert isinstance(got[0], bytes) and got[0] == _one_file(dup, gt, keep_duplicates=True) and got[2] == got[0]
    want = _gold("zero_last_%s.dnd" % gt) if gt in ("sl", "slink") else _one_file(zero_last, gt, keep_duplicates=True)
    assert _agree(got[1], want)


def test_a_heuristic_inside_a_batch():
    """-medoidtree applies to hemopexin (4188 records, threshold 2000) and not to the small families beside it."""
    hemo, adeno = os.path.join(G, "hemopexin", "hemopexin"), os.path.join(G, "adeno_fiber", "adeno_fiber")
    got = famsa_amd.guide_trees([adeno, hemo, adeno], gt="sl", heuristic="medoidtree")
    assert got[1] == _gold("hemopexin/medoid-sl.dnd")
    assert got[0] == _gold("adeno_fiber/sl.dnd") and got[2] == got[0]


def test_the_other_distance_and_a_file_named_twice():
    adeno, extra = os.path.join(G, "adeno_fiber", "adeno_fiber"), os.path.join(G, "adeno_fiber_extra", "adeno_fiber_extra")
    for gt in ("sl", "upgma"):
        got = famsa_amd.guide_trees([adeno, extra, adeno], gt=gt, distance="indel_div_lcs")
        assert got[0] == _one_file(adeno, gt, distance="indel_div_lcs") and got[2] == got[0]
        assert got[1] == _one_file(extra, gt, distance="indel_div_lcs")


def _write_list(tmp_path, paths, suffix):
    outs = [str(tmp_path / ("%02d_%s.dnd" % (k, suffix))) for k in range(len(paths))]
    lst = str(tmp_path / ("list_%s.txt" % suffix))
    with open(lst, "w") as f:
        f.write("# input<TAB>output\n\n")
        for a, b in zip(paths, outs):
            f.write("%s\t%s\n" % (a, b))
    return lst, outs


def _run(args, env_extra=None):
    env = dict(os.environ)
    env.pop("FAMSA_HOST_TEST", None)
    env.update(env_extra or {})
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)


def _check_outputs(p, rels, paths, outs, gt):
    """Every output is the wanted text; a file the one-file call refuses has an [ERROR] line and no output, and then -- only
    then -- the status is non-zero.  Returns the number of refused files."""
    refused = 0
    for rel, path, out in zip(rels, paths, outs):
        want = _want(path, rel, gt)
        if isinstance(want, Exception):
            refused += 1
            assert not os.path.exists(out), rel
            assert any(l.startswith("[ERROR] %s: " % path) and "no finite" in l for l in p.stderr.splitlines()), p.stderr[-2000:]
        else:
            assert open(out, "rb").read() == want, rel
    assert p.stderr.count("[ERROR]") == refused, p.stderr[-2000:]
    assert (p.returncode != 0) == (refused > 0), p.stderr[-2000:]
    return refused


def _totals(stderr):
    return {k: v for k, v in re.findall(r"^(batch\.\w+|time\.\w+)=(\S+)$", stderr, re.M)}


@pytest.mark.parametrize("gt", ["sl", "upgma"])
def test_cli_list_file_and_totals(tmp_path, zero_last, gt):
    paths = [os.path.join(G, rel) for rel in FILES] + [zero_last]
    lst, outs = _write_list(tmp_path, paths, gt)
    p = _run(["-gt", gt, "-gt_export", "-batch", lst, "-v"])
    refused = _check_outputs(p, FILES + ["zero_last"], paths, outs, gt)
    assert refused <= 1  # (zero_last under upgma)
    t = _totals(p.stderr)
    assert int(t["batch.files"]) == len(paths) and int(t["batch.files_failed"]) == refused
    assert int(t["batch.chunks"]) >= 1
    assert int(t["batch.files_in_chunks"]) + int(t["batch.files_one_file_route"]) == len(paths) - refused
    assert int(t["batch.files_in_chunks"]) >= 5  # the small families, whatever the routing limit sends hemopexin down
    if gt == "sl":
        assert int(t["batch.files_one_file_route"]) >= 1  # adversarial_tree: orientation-sensitive members, MSTPrim's orientation
    for key in ("time.load", "time.sort", "time.gpu_upload", "time.device", "time.newick", "time.store"):
        assert float(t[key]) >= 0.0


@pytest.mark.parametrize("gt", ["sl", "slink", "upgma"])
def test_cli_forced_chunks_and_forced_one_file_route(tmp_path, zero_last, gt):
    """batch_pairs=20000 cuts the list into several chunks, batch_group_max=64 sends the adeno files down the one-file
    route: the same bytes both ways, and the same as the plain run's."""
    paths = [os.path.join(G, rel) for rel in FILES if "hemopexin" not in rel] + [zero_last]
    texts, totals = {}, {}
    for name, hook in (("plain", None), ("chunks", "batch_pairs=20000"), ("one_file", "batch_group_max=64")):
        lst, outs = _write_list(tmp_path, paths, name)
        p = _run(["-gt", gt, "-gt_export", "-batch", lst, "-v"], {"FAMSA_HOST_TEST": hook} if hook else None)
        _check_outputs(p, [rel for rel in FILES if "hemopexin" not in rel] + ["zero_last"], paths, outs, gt)
        texts[name] = [open(o, "rb").read() if os.path.exists(o) else None for o in outs]
        totals[name] = _totals(p.stderr)
    assert texts["chunks"] == texts["plain"] and texts["one_file"] == texts["plain"]
    assert int(totals["chunks"]["batch.chunks"]) > int(totals["plain"]["batch.chunks"])
    assert int(totals["one_file"]["batch.files_one_file_route"]) >= int(totals["plain"]["batch.files_one_file_route"]) + 3


def test_files_that_fail_do_not_stop_the_others(tmp_path):
    adeno, extra = os.path.join(G, "adeno_fiber", "adeno_fiber"), os.path.join(G, "adeno_fiber_extra", "adeno_fiber_extra")
    missing, empty = str(tmp_path / "missing.fasta"), str(tmp_path / "empty.fasta")
    open(empty, "w").close()
    paths = [adeno, missing, extra, empty, adeno]
    lst, outs = _write_list(tmp_path, paths, "fail")
    p = _run(["-gt", "sl", "-gt_export", "-batch", lst, "-v"])
    assert p.returncode != 0
    errors = [l for l in p.stderr.splitlines() if l.startswith("[ERROR] ")]
    assert len(errors) == 2, p.stderr[-2000:]
    assert any(l.startswith("[ERROR] %s: " % missing) for l in errors) and any(l.startswith("[ERROR] %s: " % empty) for l in errors)
    assert open(outs[0], "rb").read() == _gold("adeno_fiber/sl.dnd") and open(outs[4], "rb").read() == _gold("adeno_fiber/sl.dnd")
    assert open(outs[2], "rb").read() == _one_file(extra, "sl")
    assert not os.path.exists(outs[1]) and not os.path.exists(outs[3])
    assert int(_totals(p.stderr)["batch.files_failed"]) == 2

    got = famsa_amd.guide_trees(paths, gt="sl", on_error="return")
    assert [isinstance(r, Exception) for r in got] == [False, True, False, True, False]
    assert str(got[1]) and str(got[3]) and got[0] == _gold("adeno_fiber/sl.dnd") and got[2] == _one_file(extra, "sl")
    with pytest.raises(RuntimeError):
        famsa_amd.guide_trees(paths, gt="sl")
