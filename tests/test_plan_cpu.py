"""The step planner (gcm_amd/csrc/plan.hpp) without a GPU: tests/plan_check.cpp,
a stand-alone program built with the address and undefined-behaviour
sanitizers, enumerates every reachable input and asserts the invariants the
executor relies on; the plans it can return are exactly those the GPU table
(tests/step_plan_table.py) exercises."""
import os
import shutil
import subprocess

import pytest

from tests import step_plan_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_check_output(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "plan_check.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_planner_invariants(plan_check_output):
    last = plan_check_output.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith(", 0 failed"), last
    assert int(last.split()[1]) > 1_000_000, last


def test_gpu_table_covers_every_reachable_plan(plan_check_output):
    reachable = sorted(l[len("plan "):] for l in plan_check_output.splitlines() if l.startswith("plan "))
    print("reachable plans:", reachable)
    assert reachable == T.expected_plans()


def test_table_is_well_formed():
    for case in T.CASES:
        for op, _, courant, plan in case.script:
            assert (courant is not None) == (op in ("step", "faces", "ode", "map", "stage")), (case, op)
            assert plan is None or op in ("step", "faces", "ode", "map"), (case, op)
