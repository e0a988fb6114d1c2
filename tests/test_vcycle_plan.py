"""The V-cycle's path decision (parelagmc_amd/csrc/vcycle_plan.hpp) against a restatement of the predicates it replaced:
tests/c/vcycle_plan_check.cpp includes that header only and needs neither the library nor a device.  It compares level_step and
cycle_role with the earlier level_path / inner_f32 / cycle_role / top_reads_r32, the row-split condition and the fp32 hand-over
of Multigrid::cycle on every combination of one level's facts, on 100 000 seeded random hierarchies and on the ten handle /
storage regimes of tests/test_gpu_sampler_precond.py, and fails unless every LevelPath and every role is reached."""
import os
import subprocess

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "c", "bin", "vcycle_plan_check")


def test_vcycle_plan_equals_the_predicates_it_replaced():
    r = subprocess.run(["make", "-C", ROOT, "test-vcycle-plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip())
    assert r.returncode == 0 and "vcycle_plan_check OK" in r.stdout, r.stdout + r.stderr
