"""Pins of the engine's set-up: what H.Engine(task) leaves on the device and what
the first two steps make of it, per body, with the node loops on the host and on
the device.

The expected values are tests/golden/setup_pins.json, recorded once by record()
below (python -m tests.test_gpu_setup_pins --record) from the host code as it was
BEFORE the set-up paths of HipMesh became one; the file is never recorded again
from later code.  What is pinned is behaviour a restructuring of the set-up could
change without any other test noticing: which conditions share a device
material, whose eigenvalues enter the time step, whether ids are set at all, and
how many bytes cross the bus."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_setup import (acoustic_task, cube_task, hidden_default_task, ortho_layers_task,
                                  stack_same_material_task, stack_task, xcontact_task)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "setup_pins.json")


def lone_same_material_task(H):
    """One body whose upper half in y is a second condition of the SAME material
    (another material number); both conditions hold nodes.  A stack would share
    the table entry; a lone body keeps two device materials and the per-node-material
    kernel."""
    from tests.taskspec import host_task, spec
    s = spec(3, 2, [1, 1, 1], {0: ([10, 12, 64], [0, 0, 0])}, 0.9, (4, 2, 1), snaps=1, steps_per_snap=2,
             quantities=[(("sphere", 4.0, (5.0, 6.0, 32.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.add_material(("box", (-1, 5.5, -1), (100, 100, 100)), 4, 2, 1, number=5)
    t.set_vtk_quantities(["PRESSURE"])
    return t, [0]


def hidden_default(H):
    return hidden_default_task(H, False), [0]


# name -> (maker, environment of the case)
CASES = {
    "cube": (cube_task, {}),
    "stack": (stack_task, {}),
    "stack_same_material": (stack_same_material_task, {}),
    "ortho_layers": (ortho_layers_task, {}),
    "acoustic": (acoustic_task, {}),
    "xcontact_no_stacks": (xcontact_task, {"GCMX_NO_STACKS": "1"}),
    "hidden_default": (hidden_default, {}),
    "lone_same_material": (lone_same_material_task, {}),
}
FLAGS = {"host": False, "device": True}


def sha(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def observe(H, make, flag, out):
    """The pinned fields of one case, {body: {field: value}}; writes its snapshots
    under the current directory."""
    from tests.helpers import read_vts
    t, bodies = make(H)
    t.set_device_setup(flag)
    t.add_snapshotter("VTK")
    t.output_directory = out
    t.number_of_snaps = 1  # run(): snapshot 0, two steps, snapshot 2
    t.steps_per_snap = 2
    e = H.Engine(t)
    res = {}
    for i in bodies:  # the transfers first: e.pde itself copies
        d2h, h2d = e.transfer_bytes(i)
        res[str(i)] = {"transfer_bytes_d2h": int(d2h), "transfer_bytes_h2d": int(h2d)}
    for i in bodies:
        r = res[str(i)]
        r["pde_after_construction"] = sha(e.pde(i))
        r["maximal_eigenvalue"] = float(e.maximal_eigenvalue(i)).hex()
        r["matrix_structure"] = int(e.matrix_structure(i))
        r["path"] = e.path(i)
        e.profile(i, True)
    e.run()
    assert e.steps == 2
    for i in bodies:
        r = res[str(i)]
        r["pde_after_2_steps"] = sha(e.pde(i))
        r["time_after_2_steps"] = float(e.time).hex()
        r["last_path"] = e.last_path(i)
        r["profile_kernels"] = sorted(e.profile_kernels(i))
        arrays = read_vts(f"snapshots/{out}/vtk/mesh{i}core00snap0000.vts")[1]
        r["material_index"] = sha(arrays["material_index"])
    return res


def record():
    """Write the golden file from the code that is built now."""
    import tempfile
    os.environ["GCMX_FP"] = "exact"  # as tests/conftest.py sets it for the suite
    from gcm_amd import _gcm_host as H
    golden = {}
    home = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for name, (make, env) in CASES.items():
                os.environ.update(env)
                for mode, flag in FLAGS.items():
                    golden[f"{name}/{mode}"] = observe(H, make, flag, mode)
                for k in env:
                    del os.environ[k]
        finally:
            os.chdir(home)
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(golden)} cases to {GOLDEN}")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("name", list(CASES))
def test_setup_is_as_pinned(golden, tmp_path, monkeypatch, name, mode):
    from gcm_amd import _gcm_host as H
    make, env = CASES[name]
    monkeypatch.chdir(tmp_path)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = golden[f"{name}/{mode}"]
    got = observe(H, make, FLAGS[mode], mode)
    assert sorted(got) == sorted(want), (name, mode, "bodies")
    for body in want:
        assert sorted(got[body]) == sorted(want[body]), (name, mode, body, "fields")
        for field in want[body]:
            print(f"{name}/{mode} body {body} {field}: {got[body][field]}")
            assert got[body][field] == want[body][field], f"{name}/{mode}, body {body}, {field}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_gpu_setup_pins --record")
    record()
