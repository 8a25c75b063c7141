"""The set-up calls by areas (gcmx_setup_state, gcmx_setup_census,
gcmx_setup_material_ids, gcmx_download_material_ids) without a GPU: the ABI
surface, the error path of a null context, the Task flag that opts an engine
into them, and that the split of buildHostState leaves host_state what it was."""
import ctypes
import os

import numpy as np

from tests.taskspec import host_task, spec
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["gcmx_setup_state", "gcmx_setup_census", "gcmx_setup_material_ids", "gcmx_download_material_ids"]


def test_symbols_in_header_binding_and_library():
    import gcm_amd
    from gcm_amd.gcmx import SYMBOLS
    declared = declared_symbols()
    assert sorted(SYMBOLS) == declared
    lib = gcm_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and s in SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.gcmx_abi_version() == 3
    text = open(os.path.join(ROOT, "include", "gcmx.h")).read()
    assert "#define GCMX_ABI_VERSION 3" in text
    assert "#define GCMX_MAX_SETUP_AREAS 256" in text
    assert gcm_amd.gcmx.MAX_SETUP_AREAS == 256


def test_struct_layouts():
    from gcm_amd import gcmx
    assert ctypes.sizeof(gcmx.Area) == 88
    assert gcmx.Area.p.offset == 8
    assert ctypes.sizeof(gcmx.SetupBox) == 36
    assert (gcmx.AREA_INFINITE, gcmx.AREA_BOX, gcmx.AREA_SPHERE, gcmx.AREA_CYLINDER) == (0, 1, 2, 3)


def test_make_area_forms_the_cylinder_axis_like_the_host():
    """The host constructor's three operations (host/task.hpp): the difference, its
    length as sqrt of the sum of squares in that association, one division each."""
    from gcm_amd import gcmx
    b, e = (0.3, -1.7, 2.9), (4.1, 0.2, 11.3)
    a = gcmx.make_area(("cylinder", 1.25, b, e))
    d = [np.float64(e[i]) - np.float64(b[i]) for i in range(3)]
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    want = [1.25, *b, *e, *[x / length for x in d]]
    assert a.kind == gcmx.AREA_CYLINDER
    assert np.array_equal(np.array(a.p[:]).view(np.uint64), np.array(want, dtype=np.float64).view(np.uint64))
    s = gcmx.make_area(("sphere", 2.0, (1.0, 2.0, 3.0)))
    assert s.kind == gcmx.AREA_SPHERE and list(s.p[:4]) == [2.0, 1.0, 2.0, 3.0]
    bx = gcmx.make_area(("box", (1, 2, 3), (4, 5, 6)))
    assert bx.kind == gcmx.AREA_BOX and list(bx.p[:6]) == [1, 2, 3, 4, 5, 6]
    assert gcmx.make_area(("infinite",)).kind == gcmx.AREA_INFINITE


def test_new_calls_fail_loudly_without_a_context():
    """A null context is an error with a message of its own, never a silent success."""
    import gcm_amd
    from gcm_amd import gcmx
    lib = gcm_amd.lib()
    area = (gcmx.Area * 1)(gcmx.make_area(("infinite",)))
    vec = (ctypes.c_double * 9)()
    ids = (ctypes.c_uint8 * 1)(0)
    used = (ctypes.c_uint32 * 8)()
    out = (ctypes.c_uint8 * 8)()
    calls = {
        "gcmx_setup_state": lambda: lib.gcmx_setup_state(None, None, 1, area, vec),
        "gcmx_setup_census": lambda: lib.gcmx_setup_census(None, None, 1, area, ids, used),
        "gcmx_setup_material_ids": lambda: lib.gcmx_setup_material_ids(None, None, 1, area, ids),
        "gcmx_download_material_ids": lambda: lib.gcmx_download_material_ids(None, out),
    }
    for name, call in calls.items():
        # the message of another failure first ("null argument"), so that a call
        # which returns an error without a message of its own is caught
        assert lib.gcmx_create(None, 0, None) != 0
        marker = lib.gcmx_last_error()
        status = call()
        assert status != 0, name
        msg = lib.gcmx_last_error()
        assert msg and msg != marker, (name, msg)
    assert not any(used) and not any(out)


def a_task(device_setup=None):
    s = spec(2, 2, [0.5, 0.25], {0: ([9, 13], [3, -2])}, 0.9, (4, 2, 1),
             inhomogeneities=[(("box", (-10, -10, -10), (4.2, 100, 100)), (2, 1, 1)),
                              (("sphere", 1.0, (3.0, 1.0, 0.0)), (3, 1, 1))], snaps=1,
             quantities=[(("sphere", 2.5, (4.0, 0.0, 3.0)), "PRESSURE", 3.0)],
             waves=[(("cylinder", 1.5, (0.0, -1.0, 0.0), (7.0, 3.0, 0.0)), "P_FORWARD", 1, "Vy", -2.0)],
             vectors=[(("box", (1, -5, -5), (6, 9, 90)), list(np.linspace(-1, 1, 5)))])
    t = host_task(s)
    if device_setup is not None:
        t.set_device_setup(device_setup)
    return t


def test_task_flag_defaults_to_off():
    from gcm_amd import _gcm_host as H
    t = H.Task()
    assert t.device_setup is False
    t.set_device_setup(True)
    assert t.device_setup is True
    t.set_device_setup(False)
    assert t.device_setup is False


def test_host_state_does_not_depend_on_the_flag():
    """host_state is the CPU restatement the GPU tests hold the device to: the flag
    must not reach it, and the split of its per-condition half must leave every
    array what it was (tests/golden/observe_2d.vts pins the bytes elsewhere)."""
    from gcm_amd import _gcm_host as H
    off, on = H.host_state(a_task(False), 0), H.host_state(a_task(True), 0)
    assert set(off) == set(on)
    for k in ("pde", "mat_ids"):
        assert off[k].shape == on[k].shape and off[k].tobytes() == on[k].tobytes(), k
    assert off["maximal_eigenvalue"] == on["maximal_eigenvalue"] and off["n_conditions"] == on["n_conditions"] == 3
    assert np.any(off["pde"] != 0) and set(np.unique(off["mat_ids"])) == {0, 1, 2}
    # and the oracle's set-up gives the same arrays
    from oracle import oracle as O
    from tests.taskspec import oracle_task
    s = spec(2, 2, [0.5, 0.25], {0: ([9, 13], [3, -2])}, 0.9, (4, 2, 1),
             inhomogeneities=[(("box", (-10, -10, -10), (4.2, 100, 100)), (2, 1, 1)),
                              (("sphere", 1.0, (3.0, 1.0, 0.0)), (3, 1, 1))], snaps=1,
             quantities=[(("sphere", 2.5, (4.0, 0.0, 3.0)), "PRESSURE", 3.0)],
             waves=[(("cylinder", 1.5, (0.0, -1.0, 0.0), (7.0, 3.0, 0.0)), "P_FORWARD", 1, "Vy", -2.0)],
             vectors=[(("box", (1, -5, -5), (6, 9, 90)), list(np.linspace(-1, 1, 5)))])
    ob = O.Engine(oracle_task(s)).bodies[0]
    assert ob.pde.tobytes() == off["pde"].tobytes()
    assert ob.mat_id.tobytes() == off["mat_ids"].tobytes()
