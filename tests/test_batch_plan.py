"""Batch mode without a GPU: the chunk planner (famsa_host_batch_plan) on hand-made size lists, the parsing of the
-batch list file, and the combinations the command line refuses before it starts the engine."""
import subprocess

import numpy as np
import pytest

from famsa_amd.hostlib import CLI, Host


@pytest.fixture(scope="module")
def host():
    return Host()


def _pairs(m):
    return m * (m - 1) // 2


def test_files_share_a_chunk_up_to_the_budget(host):
    # 10 + 10 + 10 members = 135 pairs: exactly the budget -> one chunk
    plan, chunks = host.batch_plan([10, 10, 10], [1, 1, 1], pair_budget=3 * _pairs(10), group_max=100)
    assert plan.tolist() == [0, 0, 0] and chunks == 1
    # one pair over: the third file opens the next chunk
    plan, chunks = host.batch_plan([10, 10, 10], [1, 1, 1], pair_budget=3 * _pairs(10) - 1, group_max=100)
    assert plan.tolist() == [0, 0, 1] and chunks == 2


def test_a_file_that_fills_the_budget_alone(host):
    plan, chunks = host.batch_plan([5, 20, 5, 5], [1, 1, 1, 1], pair_budget=_pairs(20), group_max=100)
    assert plan.tolist() == [0, 1, 2, 2] and chunks == 3
    # larger than the whole budget: a chunk to itself, never dropped
    plan, chunks = host.batch_plan([5, 21, 5], [1, 1, 1], pair_budget=_pairs(20), group_max=100)
    assert plan.tolist() == [0, 1, 2] and chunks == 3
    # one-sequence files have no pair and never open a chunk of their own while one is open
    plan, chunks = host.batch_plan([1, 1, 20, 1], [1, 1, 1, 1], pair_budget=_pairs(20), group_max=100)
    assert plan.tolist() == [0, 0, 0, 0] and chunks == 1


def test_an_ineligible_file_in_the_middle(host):
    plan, chunks = host.batch_plan([10, 10, 10], [1, 0, 1], pair_budget=1000, group_max=100)
    assert plan.tolist() == [0, -1, 0] and chunks == 1
    # over the routing limit counts the same, at the limit does not
    plan, chunks = host.batch_plan([10, 101, 100, 10], [1, 1, 1, 1], pair_budget=10 ** 6, group_max=100)
    assert plan.tolist() == [0, -1, 0, 0] and chunks == 1


def test_every_file_over_the_limit_and_the_empty_list(host):
    plan, chunks = host.batch_plan([65, 70, 4097], [1, 1, 1], pair_budget=10 ** 6, group_max=64)
    assert plan.tolist() == [-1, -1, -1] and chunks == 0
    plan, chunks = host.batch_plan([], [], pair_budget=10 ** 6, group_max=64)
    assert plan.tolist() == [] and chunks == 0


def test_the_limit_never_exceeds_what_one_workgroup_holds(host):
    plan, _ = host.batch_plan([4096, 4097], [1, 1], pair_budget=10 ** 9, group_max=10 ** 6)
    assert plan.tolist() == [0, -1]
    plan, chunks = host.batch_plan([2, 2000000], [1, 1])  # the defaults
    assert plan.tolist() == [0, -1] and chunks == 1


def _cli(*args, cwd=None):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=cwd)


def test_list_file_comments_and_blank_lines(tmp_path):
    """Only comments and blank lines: nothing to do, status 0, no engine needed."""
    lst = tmp_path / "list.txt"
    lst.write_text("# families of the day\n\n   \n#a.fasta\tb.dnd\n")
    p = _cli("-gt", "sl", "-gt_export", "-batch", str(lst), "-v")
    assert p.returncode == 0, p.stderr
    assert "batch.files=0" in p.stderr


def test_list_file_line_without_a_tab(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("# comment\n\na.fasta\ta.dnd\nb.fasta b.dnd\n")
    p = _cli("-gt_export", "-batch", str(lst))
    assert p.returncode != 0
    assert "line 4" in p.stderr and "[ERROR]" in p.stderr
    assert not (tmp_path / "a.dnd").exists()


def test_missing_list_file(tmp_path):
    p = _cli("-gt_export", "-batch", str(tmp_path / "nothing.txt"))
    assert p.returncode != 0 and "cannot open the batch list" in p.stderr


@pytest.mark.parametrize("extra,word", [(["-dist_export"], "-dist_export"), (["-stats", "s.txt"], "-stats"),
                                        (["-dump_seeds", "seeds.txt"], "-dump_seeds"), (["in.fasta", "out.dnd"], "in.fasta"),
                                        (["-gpus", "2"], "-gpus")])
def test_refused_combinations(tmp_path, extra, word):
    """Refused with a message that names the offender, before the engine is started: a list that names a file which does
    not exist would otherwise end in that file's error (and on a machine without a GPU in the engine's)."""
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\n" % (tmp_path / "nothing.fasta", tmp_path / "out.dnd"))
    p = _cli("-gt_export", "-batch", str(lst), *extra, cwd=str(tmp_path))
    assert p.returncode != 0
    assert "-batch" in p.stderr and word in p.stderr, p.stderr
    assert "nothing.fasta" not in p.stderr and "lcsgpu_create" not in p.stderr
    assert not (tmp_path / "s.txt").exists() and not (tmp_path / "out.dnd").exists()


def test_planner_agrees_with_a_plain_restatement(host):
    rng = np.random.Generator(np.random.PCG64(9))
    counts = rng.integers(1, 400, size=300)
    eligible = rng.random(300) < 0.9
    budget, limit = 20000, 256
    want, chunk, used = [], -1, 0
    for m, e in zip(counts.tolist(), eligible.tolist()):
        if not e or m > limit:
            want.append(-1)
            continue
        if chunk < 0 or used + _pairs(m) > budget:
            chunk, used = chunk + 1, 0
        used += _pairs(m)
        want.append(chunk)
    plan, chunks = host.batch_plan(counts, eligible, pair_budget=budget, group_max=limit)
    assert plan.tolist() == want and chunks == chunk + 1
