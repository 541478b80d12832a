"""famsa_amd/csrc/text_plan.h -- which workgroup of the batched text launches (lcsgpu_dist_text_batch) formats which value
of which list's row, and where it reads it -- replayed on the host: a wrong table is a silently wrong distance file.

The plan is plain host code, so the check is a small C++ program of its own (tests/host_src/text_plan_check.cpp, built by
famsa_amd/csrc/Makefile into famsa_amd/_build/): lists of 0, 1, 2, 1023, 1024, 1025, 2049 and random sizes, alone and mixed,
lower and square form; every (list, row, column) value owned by exactly one (job, thread, slot), every source index inside
its own list's triangle or rectangle, every row -- an empty one too -- with a first segment for its name."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "famsa_amd", "_build", "text_plan_check")


def test_text_tables_own_every_value_once():
    assert os.path.exists(CHECK), "famsa_amd/_build/text_plan_check is missing: python __graft_entry__.py builds it"
    p = subprocess.run([CHECK], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout
    assert p.stdout.startswith("ok: 22 calls, "), p.stdout
