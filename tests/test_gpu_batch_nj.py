"""Batch mode with the NJ merges on the device (lcsgpu_nj_batch: a workgroup per file) end to end:
`famsa-gpu -gt nj -gt_export -batch <list> -v` and famsa_amd.guide_trees over the golden families of
test_gpu_batch_trees.py, the three synthetic tie-heavy files of test_gpu_batch_upgma.py (257, 700 and 1025 sequences over
small alphabets: many equal float distances; 1025 is past the routing limit and joins a chunk once the limit is lifted)
and allx (half of its sequences are made of the code that matches nothing: no finite q -- that file fails, alone, in the
words of the one-file call).  Every output equals the reference-made golden where tests/golden has an `nj` one, the host
builder over the oracle's LCS matrix (pinned to the reference by the CPU suite) for the synthetic files, and the one-file
call everywhere else.  batch.files_device_nj counts the files whose merges ran on the device;
FAMSA_HOST_TEST=batch_nj_host keeps the earlier route (triangles to the host builders) and must write the same bytes."""
import os

import numpy as np
import pytest

import famsa_amd
import mst_shapes
import test_gpu_batch_trees as bt
from famsa_amd import hostlib as host_bind
from famsa_amd import seqio
from test_gpu_batch_upgma import DISTS, SYNTH

pytestmark = pytest.mark.gpu
G = bt.G
GT = "nj"
REFUSED = "allx"
_WANT = {}
_RUNS = {}


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """([(label, path)], the synthetic files' oracle matrices, {label: unique sequences}): the golden families, the synthetic
    files, allx."""
    d = tmp_path_factory.mktemp("batch_nj")
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
    refused = str(d / (REFUSED + ".fasta"))
    with open(refused, "w") as f:
        for i, s in enumerate(mst_shapes.build(REFUSED)):
            f.write(">s%d\n%s\n" % (i, "".join(seqio.ALPHABET[c] for c in s)))
    out.append((REFUSED, refused))
    host = host_bind.Host()
    unique = {label: host.workset(path, len(seqio.read_fasta(path)[0]))[0] for label, path in out}
    assert unique["synth1025"] == 1025 and 2 <= unique[REFUSED] <= 1000  # (allx goes into a chunk)
    return out, squares, unique


def _want(files, label, path, dist):
    """The wanted text of one file, or the RuntimeError of the one-file call -- made once."""
    key = (label, dist)
    if key not in _WANT:
        if dist == DISTS[0] and GT in bt.GOLD.get(label, {}):
            _WANT[key] = bt._gold(bt.GOLD[label][GT])
        elif path in files[1]:
            _WANT[key] = host_bind.Host().tree_from_matrix(path, files[1][path], GT, distance=dist)
        else:
            _WANT[key] = bt._one_file(path, GT, distance=dist)
    return _WANT[key]


@pytest.mark.parametrize("dist", DISTS)
def test_guide_trees(files, dist):
    got = famsa_amd.guide_trees([path for _, path in files[0]], gt=GT, distance=dist, on_error="return")
    bad = [label for (label, path), text in zip(files[0], got) if not bt._agree(text, _want(files, label, path, dist))]
    assert not bad, (dist, bad)
    assert [isinstance(text, Exception) for text in got] == [label == REFUSED for label, _ in files[0]]
    assert "NJ: no finite q" in str(got[-1]) and "NJ: no finite q" in str(_want(files, REFUSED, files[0][-1][1], dist))


def _with_merges(files, group_max):
    """The files of the command-line runs that a chunk takes, that have a tree stage, and that have a tree."""
    return [label for label, _ in files[0] if "hemopexin" not in label and label != REFUSED and 2 <= files[2][label] <= group_max]


def _cli(files, tmp_path_factory, dist, hook):
    """One run of the command-line tool over the list (without hemopexin: 4188 records take the one-file route) --
    (texts, totals), made once per setting."""
    key = (dist, hook)
    if key not in _RUNS:
        chosen = [(label, path) for label, path in files[0] if "hemopexin" not in label]
        d = tmp_path_factory.mktemp("cli")
        lst, outs = bt._write_list(d, [path for _, path in chosen], "n")
        p = bt._run(["-gt", GT, "-dist", dist, "-gt_export", "-batch", lst, "-v"], {"FAMSA_HOST_TEST": hook} if hook else None)
        texts = []
        for (label, path), out in zip(chosen, outs):
            want = _want(files, label, path, dist)
            if isinstance(want, Exception):
                assert label == REFUSED and not os.path.exists(out)
                assert any(l.startswith("[ERROR] %s: " % path) and "NJ: no finite q" in l for l in p.stderr.splitlines()), p.stderr[-2000:]
                texts.append(None)
            else:
                assert os.path.exists(out), (label, p.stderr[-2000:])
                texts.append(open(out, "rb").read())
                assert texts[-1] == want, label
        assert p.stderr.count("[ERROR]") == 1 and p.returncode != 0, p.stderr[-2000:]  # allx, alone
        _RUNS[key] = (texts, {k: int(v) for k, v in bt._totals(p.stderr).items() if k.startswith("batch.")})
    return _RUNS[key]


@pytest.mark.parametrize("dist", DISTS)
def test_cli_counts_the_files_whose_merges_ran_on_the_device(files, tmp_path_factory, dist):
    texts, t = _cli(files, tmp_path_factory, dist, None)
    assert t["batch.files_device_nj"] > 0
    # every file a chunk took and finished had its merges on the device (one unique sequence: no tree stage, no merges)
    assert t["batch.files_device_nj"] == len(_with_merges(files, 1000))
    assert t["batch.files_device_upgma"] == 0
    assert t["batch.files_one_file_route"] == 1 and t["batch.files_failed"] == 1  # synth1025 is past the routing limit; allx


@pytest.mark.parametrize("dist", DISTS)
def test_cli_host_builders_write_the_same_bytes(files, tmp_path_factory, dist):
    texts, t = _cli(files, tmp_path_factory, dist, "batch_nj_host")
    assert t["batch.files_device_nj"] == 0
    assert texts == _cli(files, tmp_path_factory, dist, None)[0]


@pytest.mark.parametrize("dist", DISTS)
def test_cli_the_routing_limit_lifted(files, tmp_path_factory, dist):
    """batch_group_max=4096: the 1025-member file joins the chunk and its merges run on the device as well."""
    texts, t = _cli(files, tmp_path_factory, dist, "batch_group_max=4096")
    plain = _cli(files, tmp_path_factory, dist, None)
    assert t["batch.files_one_file_route"] == 0
    assert t["batch.files_device_nj"] == len(_with_merges(files, 4096)) == plain[1]["batch.files_device_nj"] + 1
    assert texts == plain[0]


@pytest.mark.parametrize("dist", DISTS)
def test_cli_several_chunks(files, tmp_path_factory, dist):
    texts, t = _cli(files, tmp_path_factory, dist, "batch_pairs=20000")
    plain = _cli(files, tmp_path_factory, dist, None)
    assert t["batch.chunks"] > plain[1]["batch.chunks"]
    assert t["batch.files_device_nj"] == plain[1]["batch.files_device_nj"]
    assert texts == plain[0]
