"""Save and resume through the engine (Engine::saveState / loadState, the state by
boxes underneath).  Engine A runs 6 steps.  Engine B runs 3, saves and is dropped.
Engine C is built from the same task, loads the file and runs 3.  A and C must
agree on every body's pde (bit for bit, ghosts included), steps, time and the
path of the last step, in the exact and in the FMA build of the one-pass step."""
import os

import numpy as np
import pytest

from tests.taskspec import host_task, spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {at}: "
                             f"got {got[at]!r} want {want[at]!r}")


def bits_of(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


# ---------------------------------------------------------------- the cases --

FREE = {0: ("Sxx", "Sxy", "Sxz"), 1: ("Sxy", "Syy", "Syz"), 2: ("Sxz", "Syz", "Szz")}


def iso3_task(device_setup):
    """3-D isotropic, free surfaces on all faces, Maxwell ODE, two materials by areas."""
    def make():
        s = spec(3, 2, [1, 1, 1], {0: ([12, 10, 70], [0, 0, 0])}, 0.9, (4, 2, 1, 0.7), snaps=6,
                 inhomogeneities=[(("box", (-1, -1, 30.5), (100, 100, 100)), (2, 1, 1, 1.3))],
                 quantities=[(("sphere", 4.0, (6.0, 5.0, 33.0)), "PRESSURE", 10.0)],
                 borders={0: [(d, ("infinite",), {q: (lambda t: 0.0) for q in FREE[d]}) for d in range(3)]},
                 odes={0: ["MAXWELL_VISCOSITY"]})
        t = host_task(s)
        t.set_device_setup(device_setup)
        return t
    return make, [0], False, {}


def stack_task():
    """Two bodies stacked along y with a contact: one grid."""
    def make():
        cubics = {0: ([10, 5, 64], [0, 0, 0]), 1: ([10, 7, 64], [0, 5, 0])}
        s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=6,
                 inhomogeneities=[(("box", (-1, 8.5, -1), (100, 100, 100)), (2, 1, 1))],
                 quantities=[(("sphere", 5.0, (5.0, 3.5, 32.0)), "PRESSURE", 10.0)])
        return host_task(s)
    return make, [0, 1], True, {}


def xcontact_task():
    """Two bodies with a contact along x, run as two grids (GCMX_NO_STACKS=1): a
    contact copy fills the ghosts before every x stage."""
    def make():
        cubics = {0: ([12, 9, 64], [0, 0, 0]), 1: ([12, 9, 64], [12, 0, 0])}
        s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=6,
                 quantities=[(("sphere", 6.0, (10.5, 4.5, 32.0)), "PRESSURE", 10.0)])
        return host_task(s)
    return make, [0, 1], False, {"GCMX_NO_STACKS": "1"}


def acoustic_task(sizes=(20, 70), model="acoustic"):
    """The reference's 2-D acoustic launcher task, smaller: PRESSURE = 0 on the y- face."""
    def make():
        from gcm_amd import _gcm_host as H
        t = H.Task()
        t.dimensionality = 2
        t.border_size = 2
        t.h = [1.0, 1.0]
        t.courant = 1.0
        t.number_of_snaps = 6
        t.add_body(0, list(sizes), [0, 0], model=model)
        t.set_default_material(1.0, 1.0, 0.0 if model == "acoustic" else 0.5)
        t.add_initial_quantity(("sphere", 6.0, (10.0, 30.0, 0.0)), "PRESSURE", 10.0)
        if model == "acoustic":
            t.add_border_condition(0, 1, ("box", (-1e3, -1e3, -1e3), (1e3, 1e-5, 1e3)), {"PRESSURE": lambda time: 0.0})
        return t
    return make, [0], False, {}


def line_task():
    def make():
        s = spec(1, 2, [0.5], {0: ([100], [0])}, 0.9, (4, 2, 1), snaps=6,
                 waves=[(("box", (10, -1, -1), (20, 1, 1)), "P_FORWARD", 0, "PRESSURE", 1.0)])
        return host_task(s)
    return make, [0], False, {}


CASES = {"iso3 device set-up": iso3_task(True), "iso3 host set-up": iso3_task(False), "y stack": stack_task(),
         "x contact": xcontact_task(), "acoustic 2-D": acoustic_task(), "elastic 1-D": line_task()}


def state_of(e, bodies):
    return {"pde": {i: e.pde(i) for i in bodies}, "steps": e.steps, "time": bits_of(e.time),
            "path": {i: e.last_path(i) for i in bodies}}


def inner_bytes(pde, bs=2):
    return int(np.prod([n - 2 * bs for n in pde.shape[:-1]])) * pde.shape[-1] * 8


@pytest.mark.parametrize("fp", ["exact", "fma"])
@pytest.mark.parametrize("case", list(CASES))
def test_resume_equals_the_uninterrupted_run(H, tmp_path, monkeypatch, case, fp):
    make, bodies, one_grid, env = CASES[case]
    monkeypatch.setenv("GCMX_FP", fp)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = str(tmp_path / "state.gcmx")

    a = H.Engine(make())
    a.run_steps(6)
    A = state_of(a, bodies)
    assert all(np.any(p != 0) and np.isfinite(p).all() for p in A["pde"].values())
    del a

    b = H.Engine(make())
    b.run_steps(3)
    mid = state_of(b, bodies)
    before = {i: b.transfer_bytes(i) for i in bodies}
    b.save_state(path)
    moved = {i: inner_bytes(mid["pde"][i]) for i in bodies}
    for i in bodies:  # the bodies of one grid share its context's counters
        want = sum(moved.values()) if one_grid else moved[i]
        after = b.transfer_bytes(i)
        assert after[0] - before[i][0] == want and after[1] == before[i][1], (case, i)
    assert os.path.getsize(path) == 48 + sum(32 + m for m in moved.values())
    assert os.listdir(tmp_path) == ["state.gcmx"]
    if one_grid:  # a member's pde moves its own all-nodes box, not the stack
        before_pde = b.transfer_bytes(1)[0]
        p = b.pde(1)
        assert 0 < b.transfer_bytes(1)[0] - before_pde <= p.size * 8
    del b

    c = H.Engine(make())
    before = {i: c.transfer_bytes(i) for i in bodies}
    c.load_state(path)
    for i in bodies:
        want = sum(moved.values()) if one_grid else moved[i]
        after = c.transfer_bytes(i)
        assert after[1] - before[i][1] == want and after[0] == before[i][0], (case, i)
    assert c.steps == 3 and bits_of(c.time) == mid["time"]
    for i in bodies:  # the inner nodes are the saved ones
        idx = tuple(slice(2, -2) for _ in mid["pde"][i].shape[:-1])
        same_bits(c.pde(i)[idx], mid["pde"][i][idx], f"{case} {fp} body {i} after the load")
    c.run_steps(3)
    C = state_of(c, bodies)
    assert C["steps"] == A["steps"] == 6 and C["time"] == A["time"]
    assert C["path"] == A["path"], (case, fp, C["path"], A["path"])
    for i in bodies:
        same_bits(C["pde"][i], A["pde"][i], f"{case} {fp} body {i} after 6 steps")


def test_refusals_leave_the_engine_untouched(H, tmp_path):
    files = {}
    for name, (sizes, model) in {"sizes": ((21, 70), "acoustic"), "model": ((20, 70), "elastic")}.items():
        e = H.Engine(acoustic_task(sizes, model)[0]())
        e.run_steps(1)
        files[name] = str(tmp_path / f"{name}.gcmx")
        e.save_state(files[name])
        del e
    e = H.Engine(acoustic_task()[0]())
    e.run_steps(2)
    own = str(tmp_path / "own.gcmx")
    e.save_state(own)
    files["truncated"] = str(tmp_path / "cut.gcmx")
    with open(own, "rb") as f:
        raw = f.read()
    with open(files["truncated"], "wb") as f:
        f.write(raw[:-1])
    e.run_steps(1)
    before = state_of(e, [0])
    moved = e.transfer_bytes(0)
    for name, path in files.items():
        with pytest.raises(H.GcmException) as err:
            e.load_state(path)
        assert name in str(err.value), (name, str(err.value))
        after = state_of(e, [0])
        same_bits(after["pde"][0], before["pde"][0], f"pde after the refused {name} file")
        assert after["steps"] == before["steps"] == 3 and after["time"] == before["time"]
    assert e.transfer_bytes(0)[1] == moved[1]
    with pytest.raises(H.GcmException):
        e.load_state(str(tmp_path / "absent.gcmx"))
    # and the own file still loads
    e.load_state(own)
    assert e.steps == 2


def cube_task(snaps, out):
    s = spec(3, 2, [1, 1, 1], {0: ([12] * 3, [0] * 3)}, 0.9, (4, 2, 1), snaps=snaps, steps_per_snap=2,
             quantities=[(("sphere", 3.0, (6.0, 6.0, 6.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_vtk_quantities(["PRESSURE", "Vx"])
    t.add_snapshotter("VTK")
    t.output_directory = out
    t.set_checkpoint("checkpoints/" + out, 2)
    return t


def snapshot_files(out):
    d = f"snapshots/{out}/vtk"
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


@pytest.mark.parametrize("fp", ["exact", "fma"])
def test_run_resumes_from_its_checkpoint(H, tmp_path, monkeypatch, fp):
    """run() with VTK snapshots and a checkpoint every 2 steps: 6 steps at once
    against 4 steps, a new engine, load_state and run().  The second engine writes
    into a directory of its own, so every file it writes is seen: only the
    snapshot of step 6, and the two directories together are the baseline's."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("GCMX_FP", fp)
    base = H.Engine(cube_task(3, "base"))
    assert base.checkpoint_file == "checkpoints/base/checkpoint.gcmx"
    base.run()
    assert base.steps == 6
    want = {"pde": base.pde(0), "time": bits_of(base.time), "path": base.last_path(0)}
    del base
    baseline = snapshot_files("base")
    assert sorted(baseline) == [f"mesh0core00snap{s:04d}.vts" for s in (0, 2, 4, 6)]
    assert H.state_file_read("checkpoints/base/checkpoint.gcmx")["steps"] == 6
    assert os.listdir("checkpoints/base") == ["checkpoint.gcmx"]

    first = H.Engine(cube_task(2, "first"))
    first.run()
    assert first.steps == 4
    del first
    assert H.state_file_read("checkpoints/first/checkpoint.gcmx")["steps"] == 4

    second = H.Engine(cube_task(3, "second"))
    second.load_state("checkpoints/first/checkpoint.gcmx")
    assert second.steps == 4
    second.run()
    assert second.steps == 6 and bits_of(second.time) == want["time"] and second.last_path(0) == want["path"]
    same_bits(second.pde(0), want["pde"], f"pde after the resumed run, {fp}")
    got_first, got_second = snapshot_files("first"), snapshot_files("second")
    assert sorted(got_first) == [f"mesh0core00snap{s:04d}.vts" for s in (0, 2, 4)]
    assert sorted(got_second) == ["mesh0core00snap0006.vts"]  # nothing written twice
    assert {**got_first, **got_second} == baseline
    assert H.state_file_read("checkpoints/second/checkpoint.gcmx")["steps"] == 6
