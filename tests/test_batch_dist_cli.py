"""`famsa-gpu -dist_export -batch <list>` without a GPU: the list file's parsing, and what the command line refuses before
it starts the engine."""
import subprocess

import pytest

from famsa_amd.hostlib import CLI


def _cli(*args, cwd=None):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=cwd)


def test_an_empty_list_needs_no_engine(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("# matrices of the day\n\n   \n#a.fasta\tb.csv\n")
    p = _cli("-dist_export", "-square_matrix", "-batch", str(lst), "-v")
    assert p.returncode == 0, p.stderr
    assert "batch.files=0" in p.stderr and "batch.text_bytes=0" in p.stderr and "time.store=" in p.stderr


def test_a_line_without_a_tab_is_named_by_its_number(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("# comment\n\na.fasta\ta.csv\nb.fasta b.csv\n")
    p = _cli("-dist_export", "-batch", str(lst))
    assert p.returncode != 0
    assert "line 4" in p.stderr and "[ERROR]" in p.stderr
    assert not (tmp_path / "a.csv").exists()


def test_batch_needs_one_of_the_exports(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\n" % (tmp_path / "nothing.fasta", tmp_path / "out.csv"))
    p = _cli("-batch", str(lst), "-v")
    assert p.returncode != 0
    assert "-batch" in p.stderr and "-gt_export" in p.stderr and "-dist_export" in p.stderr, p.stderr
    assert "nothing.fasta" not in p.stderr and "lcsgpu_create" not in p.stderr


@pytest.mark.parametrize("extra,word", [(["-stats", "s.txt"], "-stats"), (["in.fasta", "out.csv"], "in.fasta")])
def test_refused_before_the_engine_starts(tmp_path, extra, word):
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\n" % (tmp_path / "nothing.fasta", tmp_path / "out.csv"))
    p = _cli("-dist_export", "-batch", str(lst), *extra, cwd=str(tmp_path))
    assert p.returncode != 0
    assert "-batch" in p.stderr and word in p.stderr, p.stderr
    assert "nothing.fasta" not in p.stderr and "lcsgpu_create" not in p.stderr
    assert not (tmp_path / "s.txt").exists() and not (tmp_path / "out.csv").exists()
