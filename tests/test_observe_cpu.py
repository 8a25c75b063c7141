"""The observation calls (gcmx_gather, gcmx_snapshot_box, gcmx_scan,
gcmx_transfer_stats) without a GPU: the ABI surface, the error paths, and the
GPU-free VtkSnapshotter writer, whose files must stay byte for byte what they
were before its array loop and its file writer were separated
(tests/golden/observe_*.vts were written by the unsplit writer)."""
import ctypes
import os

import numpy as np
import pytest

from tests.taskspec import host_task, spec
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

NEW_SYMBOLS = ["gcmx_node_list_create", "gcmx_node_list_destroy", "gcmx_gather", "gcmx_snapshot_box",
               "gcmx_scan", "gcmx_transfer_stats"]


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def test_symbols_match_the_header_and_abi_stays_3():
    import gcm_amd
    from gcm_amd.gcmx import SYMBOLS
    assert sorted(SYMBOLS) == declared_symbols()
    lib = gcm_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in SYMBOLS and hasattr(lib, s), s
        if s != "gcmx_node_list_destroy":
            assert getattr(lib, s).argtypes is not None, s
    assert lib.gcmx_abi_version() == 3
    assert gcm_amd.gcmx.Q_COMPONENT(0) == 64 and gcm_amd.gcmx.Q_COMPONENT(8) == 72
    text = open(os.path.join(ROOT, "include", "gcmx.h")).read()
    assert "#define GCMX_Q_COMPONENT(c) (64 + (c))" in text
    assert "#define GCMX_ABI_VERSION 3" in text


def test_new_calls_fail_loudly_without_a_context():
    """A null context (all a CPU-only host can offer: gcmx_create fails there) is
    an error with a message, never a silent success."""
    import gcm_amd
    lib = gcm_amd.lib()
    nodes = (ctypes.c_int * 3)(0, 0, 0)
    qs = (ctypes.c_int * 1)(2)
    out_d = (ctypes.c_double * 4)()
    out_f = (ctypes.c_float * 12)()
    handle = ctypes.c_void_p()
    lo, hi = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(1, 1, 1)
    res = gcm_amd.gcmx.ScanResult()
    stats = (ctypes.c_uint64 * 2)()
    calls = {
        "gcmx_node_list_create": lambda: lib.gcmx_node_list_create(None, 1, nodes, ctypes.byref(handle)),
        "gcmx_gather": lambda: lib.gcmx_gather(None, None, 1, qs, out_d),
        "gcmx_snapshot_box": lambda: lib.gcmx_snapshot_box(None, lo, hi, 1, 1, qs, out_f, out_f),
        "gcmx_scan": lambda: lib.gcmx_scan(None, ctypes.byref(res)),
        "gcmx_transfer_stats": lambda: lib.gcmx_transfer_stats(None, stats),
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
    assert not handle.value
    lib.gcmx_node_list_destroy(None)  # a null list is a no-op
    import torch
    if torch.cuda.device_count() == 0:
        with pytest.raises(gcm_amd.GcmxError):
            gcm_amd.Context(3, 2, [8, 8, 8])


def exact_layer(shape):
    """A layer of exactly representable values that needs no random generator."""
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.int64) * 2654435761) % (1 << 20)
    return ((k - (1 << 19)).astype(np.float64) / 1024.0).reshape(shape)


def case_2d():
    s = spec(2, 2, [0.5, 0.25], {0: ([9, 13], [3, -2])}, 0.9, (4, 2, 1),
             inhomogeneities=[(("box", (-10, -10, -10), (4.2, 100, 100)), (2, 1, 1))], snaps=1,
             quantities=[(("sphere", 2.5, (4.0, 0.0, 3.0)), "PRESSURE", 3.0)],
             vectors=[(("box", (1, -5, -5), (6, 9, 90)), list(np.linspace(-1, 1, 5)))])
    t = host_task(s)
    t.set_vtk_quantities(["Sxy", "PRESSURE"])
    return t, None, "observe_2d.vts"


def case_3d():
    s = spec(3, 2, [1, 1, 1], {0: ([5, 6, 7], [0, 0, 0])}, 0.9, (4, 2, 1), snaps=1)
    t = host_task(s)
    t.set_default_material(4, 2, 1, number=3)
    t.add_material(("box", (-1, -1, -1), (2.5, 100, 100)), 1, 1, 1, number=8)
    t.set_vtk_quantities(["Vz", "Syz", "PRESSURE"])
    return t, exact_layer((9, 10, 11, 9)), "observe_3d.vts"


@pytest.mark.parametrize("case", [case_2d, case_3d])
def test_split_writer_keeps_the_files_bytes(H, case, tmp_path):
    t, layer, name = case()
    path = str(tmp_path / name)
    if layer is None:
        H.write_vtk(t, 0, path)
    else:
        H.write_vtk(t, 0, path, layer)
    got = open(path, "rb").read()
    want = open(os.path.join(GOLDEN, name), "rb").read()
    assert got == want, f"{name}: {len(got)} bytes written, {len(want)} expected"
