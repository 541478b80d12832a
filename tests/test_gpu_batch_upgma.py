"""Batch mode with the UPGMA merges on the device (lcsgpu_upgma_batch: a workgroup per file) end to end:
`famsa-gpu -gt upgma|upgma_modified -gt_export -batch <list> -v` and famsa_amd.guide_trees over the golden families of
test_gpu_batch_trees.py, three synthetic tie-heavy files of 257, 700 and 1025 sequences (small alphabets: many equal
float distances; 1025 is past the routing limit and, once the limit is lifted, past the 256-thread workgroup) and
zero_last (no finite nearest neighbour: that file fails, alone).  Every output equals the reference-made golden where
tests/golden has one, the host builder over the oracle's LCS matrix (pinned to the reference by the CPU suite) for the
synthetic files, and the one-file call everywhere else.  batch.files_device_upgma counts the files whose merges ran on
the device; FAMSA_HOST_TEST=batch_upgma_host keeps the earlier route (triangles to the host builders) and must write the
same bytes."""
import os

import numpy as np
import pytest

import famsa_amd
import mst_shapes
import test_gpu_batch_trees as bt
from famsa_amd import hostlib as host_bind
from famsa_amd import seqio

pytestmark = pytest.mark.gpu
G = bt.G
GTS = ["upgma", "upgma_modified"]
DISTS = ["indel075_div_lcs", "indel_div_lcs"]
SYNTH = [(257, 1, 20, "ACD"), (700, 1, 60, "ACDE"), (1025, 14, 40, "ACDE")]  # (sequences, lengths from .. to, alphabet)
_WANT = {}
_RUNS = {}


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """([(label, path)], the synthetic files' oracle matrices, {label: unique sequences}): the golden families, the synthetic
    files, zero_last."""
    d = tmp_path_factory.mktemp("batch_upgma")
    out = [(rel, os.path.join(G, rel)) for rel in bt.FILES]
    squares = {}
    for seed, (n, min_len, max_len, alpha) in enumerate(SYNTH):
        rng = np.random.Generator(np.random.PCG64(900 + seed))
        seqs = ["".join(alpha[i] for i in rng.integers(0, len(alpha), size=int(rng.integers(min_len, max_len + 1)))) + "A" for _ in range(n)]
        path = str(d / ("synth%d.fasta" % n))
        with open(path, "w") as f:
            for i, s in enumerate(seqs):
                f.write(">r%d\n%s\n" % (i, s))
        codes, offsets = seqio.pack([oracle.encode(s) for s in seqs])
        squares[path] = oracle.rect(codes, offsets, np.arange(n), np.arange(n))
        out.append(("synth%d" % n, path))
    zero_last = str(d / "zero_last.fasta")
    mst_shapes.write_zero_last_fasta(zero_last)
    out.append(("zero_last", zero_last))
    host = host_bind.Host()
    unique = {label: host.workset(path, len(seqio.read_fasta(path)[0]))[0] for label, path in out}
    assert unique["synth1025"] == 1025  # (no duplicates: the file needs the 1024-thread workgroup)
    return out, squares, unique


def _want(files, label, path, gt, dist):
    """The wanted text of one file, or the RuntimeError of the one-file call -- made once."""
    key = (label, gt, dist)
    if key not in _WANT:
        if dist == DISTS[0] and gt in bt.GOLD.get(label, {}):
            _WANT[key] = bt._gold(bt.GOLD[label][gt])
        elif path in files[1]:
            _WANT[key] = host_bind.Host().tree_from_matrix(path, files[1][path], gt, distance=dist)
        else:
            _WANT[key] = bt._one_file(path, gt, distance=dist)
    return _WANT[key]


def _only_zero_last_fails(files, got, gt, dist):
    bad = [label for (label, path), text in zip(files[0], got) if not bt._agree(text, _want(files, label, path, gt, dist))]
    assert not bad, (gt, dist, bad)
    assert [isinstance(text, Exception) for text in got] == [label == "zero_last" for label, _ in files[0]]
    assert "no finite" in str(got[-1])


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("gt", GTS)
def test_guide_trees(files, gt, dist):
    got = famsa_amd.guide_trees([path for _, path in files[0]], gt=gt, distance=dist, on_error="return")
    _only_zero_last_fails(files, got, gt, dist)


def _with_merges(files, group_max):
    """The files of the command-line runs that a chunk takes, that have a tree stage, and that have a tree."""
    return [label for label, _ in files[0] if "hemopexin" not in label and label != "zero_last" and 2 <= files[2][label] <= group_max]


def _cli(files, tmp_path_factory, gt, dist, hook):
    """One run of the command-line tool over the list (without hemopexin: 4188 records take the one-file route or a
    workgroup of their own for seconds) -- (texts, totals), made once per setting."""
    key = (gt, dist, hook)
    if key not in _RUNS:
        chosen = [(label, path) for label, path in files[0] if "hemopexin" not in label]
        d = tmp_path_factory.mktemp("cli")
        lst, outs = bt._write_list(d, [path for _, path in chosen], "u")
        p = bt._run(["-gt", gt, "-dist", dist, "-gt_export", "-batch", lst, "-v"], {"FAMSA_HOST_TEST": hook} if hook else None)
        texts = []
        for (label, path), out in zip(chosen, outs):
            want = _want(files, label, path, gt, dist)
            if isinstance(want, Exception):
                assert label == "zero_last" and not os.path.exists(out)
                assert any(l.startswith("[ERROR] %s: " % path) and "no finite" in l for l in p.stderr.splitlines()), p.stderr[-2000:]
                texts.append(None)
            else:
                assert os.path.exists(out), (label, p.stderr[-2000:])
                texts.append(open(out, "rb").read())
                assert texts[-1] == want, label
        assert p.stderr.count("[ERROR]") == 1 and p.returncode != 0, p.stderr[-2000:]  # zero_last, alone
        _RUNS[key] = (texts, {k: int(v) for k, v in bt._totals(p.stderr).items() if k.startswith("batch.")})
    return _RUNS[key]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("gt", GTS)
def test_cli_counts_the_files_whose_merges_ran_on_the_device(files, tmp_path_factory, gt, dist):
    texts, t = _cli(files, tmp_path_factory, gt, dist, None)
    assert t["batch.files_device_upgma"] > 0
    # every file a chunk took and finished had its merges on the device (one unique sequence: no tree stage, no merges)
    assert t["batch.files_device_upgma"] == len(_with_merges(files, 1000))
    assert t["batch.files_one_file_route"] == 1 and t["batch.files_failed"] == 1  # synth1025 is past the routing limit; zero_last


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("gt", GTS)
def test_cli_host_builders_write_the_same_bytes(files, tmp_path_factory, gt, dist):
    texts, t = _cli(files, tmp_path_factory, gt, dist, "batch_upgma_host")
    assert t["batch.files_device_upgma"] == 0
    assert texts == _cli(files, tmp_path_factory, gt, dist, None)[0]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("gt", GTS)
def test_cli_the_wide_workgroup(files, tmp_path_factory, gt, dist):
    """batch_group_max=4096: the 1025-member file joins the chunk, whose launch then runs 1024-thread workgroups."""
    texts, t = _cli(files, tmp_path_factory, gt, dist, "batch_group_max=4096")
    plain = _cli(files, tmp_path_factory, gt, dist, None)
    assert t["batch.files_one_file_route"] == 0
    assert t["batch.files_device_upgma"] == len(_with_merges(files, 4096)) == plain[1]["batch.files_device_upgma"] + 1
    assert texts == plain[0]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("gt", GTS)
def test_cli_several_chunks(files, tmp_path_factory, gt, dist):
    texts, t = _cli(files, tmp_path_factory, gt, dist, "batch_pairs=20000")
    plain = _cli(files, tmp_path_factory, gt, dist, None)
    assert t["batch.chunks"] > plain[1]["batch.chunks"]
    assert t["batch.files_device_upgma"] == plain[1]["batch.files_device_upgma"]
    assert texts == plain[0]
