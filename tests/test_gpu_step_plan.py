"""The step dispatch reproduces its recorded table (tests/step_plan_table.py,
tests/golden/step_plan.json: recorded from the library of the commit before
the step planner): per call the status, the paths, the folded-ODE flag, the
profile's buckets and kernels, and in the exact build the state's SHA-256."""
import json

import pytest

from tests import step_plan_table as T

pytestmark = pytest.mark.gpu

KERNEL_OF = {"Tx2": ("k_step_tx2<", "k_fused_xyz<", "k_zseam"), "Ortho": ("k_step_ortho<",),
             "Acoustic": ("k_step_acoustic<",), "Step2d": ("k_step2d",)}
STEP_BUCKETS = ("fused_xyz", "fused_xyz_boundary", "step2d", "stage_generic", "march_x", "march_y", "line_z")


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN) as fh:
        return json.load(fh)


def check_plan(case, records):
    """Each step call's record is what its expected plan (plan.hpp) implies."""
    n = len(case.slabs or (1,))
    for i, (op, _, _, plan) in enumerate(case.script):
        if plan is None:
            continue
        kind, _, ode = plan.split()
        for rec in records[i * n:(i + 1) * n]:
            what = f"{case.name} call {i} ({op}): {rec}"
            assert rec["status"] == 0, what
            assert (rec["last_path"] == "fused") == (kind != "Stages"), what
            assert rec["ode_fused"] == (ode == "ode"), what
            steps = [k.split(":", 1) for k in rec["kernels"] if k.split(":", 1)[0] in STEP_BUCKETS]
            assert steps, what
            for bucket, kernel in steps:
                if kind == "Stages":
                    assert bucket in ("stage_generic", "march_x", "march_y", "line_z"), what
                else:
                    assert kernel.startswith(KERNEL_OF[kind]), what


@pytest.mark.parametrize("fp", ["fma", "exact"])
@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_step_plan_table(G, golden, case, fp):
    got = T.run_case(G, case, {"fma": G.FP_FMA, "exact": G.FP_EXACT}[fp])
    want = golden[f"{case.name}/{fp}"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case.name}/{fp}: record {i} (call {case.script[i // len(case.slabs or (1,))][:3]})"
    assert len(got) == len(want)
    check_plan(case, got)
