"""famsa_amd/csrc/job_plan.h -- which cells of which triangle or rectangle a workgroup of the batched LCS launches computes
and where it writes them -- replayed on the host: a wrong job table is a silently wrong tree.

The planner is plain host code, so the check is a small C++ program of its own (tests/host_src/job_plan_check.cpp, built by
famsa_amd/csrc/Makefile into famsa_amd/_build/): triangles and rectangles over units of 0 .. 600 members or columns, four
class mixes, three refs-per-workgroup policies; every ref in one bucket of the right kernel, the jobs a partition of the
refs that tiles their columns, every output cell written exactly once by the kernel's index formula."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "famsa_amd", "_build", "job_plan_check")


def test_job_tables_write_every_cell_once():
    assert os.path.exists(CHECK), "famsa_amd/_build/job_plan_check is missing: python __graft_entry__.py builds it"
    p = subprocess.run([CHECK], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout
    assert p.stdout.startswith("ok: 24 plans, "), p.stdout
