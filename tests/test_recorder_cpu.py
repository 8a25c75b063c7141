"""The recorder without a GPU: tests/receiver_check.cpp, a stand-alone program
built with the address and undefined-behaviour sanitizers, checks the point
receivers' corner and weight rule (gcm_amd/csrc/observe.hpp); the numpy
restatement the GPU tests compare with (tests/recorder_ref.py) is held to the
same cases; the C ABI declares and binds the seven recorder calls; the host
mirror's task settings validate their input."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import recorder_ref as R
from tests.test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORDER_SYMBOLS = ["gcmx_recorder_create", "gcmx_recorder_create_points", "gcmx_recorder_destroy", "gcmx_record",
                    "gcmx_recorder_count", "gcmx_recorder_read", "gcmx_recorder_reset"]


def test_receiver_rule_stand_alone(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "receiver_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "receiver_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith(", 0 failed"), last
    assert int(last.split()[1].rstrip(",")) > 300, last


def test_numpy_restatement_on_the_same_cases():
    sizes = [7, 2, 5]
    for dim in (1, 2, 3):
        s = sizes[:dim]
        base, w = R.corners(s, [3.0, 0.0, 2.0][:dim])  # on a node
        assert base == [3, 0, 2][:dim] and w[0] == 1.0 and not any(w[1:])
        base, w = R.corners(s, [6.0, 1.0, 4.0][:dim])  # the upper edge
        assert base == [5, 0, 3][:dim] and w[-1] == 1.0 and not any(w[:-1])
        base, w = R.corners(s, [2.25, 0.625, 3.9][:dim])
        assert base == [2, 0, 3][:dim]
        t = [0.25, 0.625, 3.9 - 3.0][:dim]
        for k in range(1 << dim):
            want = None
            for d in range(dim):
                f = t[d] if (k >> (dim - 1 - d)) & 1 else 1.0 - t[d]
                want = f if want is None else want * f
            assert w[k] == want
        assert R.corner_index(dim, base, 1) == tuple(b + (d == dim - 1) for d, b in enumerate(base))
        for d in range(dim):
            for bad in (float("nan"), -0.5, float(s[d]), np.nextafter(float(s[d] - 1), np.inf), float("inf")):
                pos = [1.0, 0.5, 1.0][:dim]
                pos[d] = bad
                assert R.corners(s, pos) is None
            one = list(s)
            one[d] = 1
            assert R.corners(one, [0.0] * dim) is None


def test_abi_declares_and_binds_the_recorder():
    import gcm_amd
    from gcm_amd.gcmx import SYMBOLS
    lib = gcm_amd.lib()
    declared = declared_symbols()
    for s in RECORDER_SYMBOLS:
        assert s in declared, s
        assert s in SYMBOLS, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes, s
    assert lib.gcmx_abi_version() == 3  # symbols are only added
    assert lib.gcmx_recorder_destroy.restype is None
    assert lib.gcmx_recorder_count.restype is ctypes.c_int
    # without a device: the argument checks that need none
    assert lib.gcmx_recorder_count(None) == 0
    out = (ctypes.c_double * 1)()
    assert lib.gcmx_recorder_read(None, 0, 1, out) == 1  # GCMX_ERR_INVALID_ARG
    assert lib.gcmx_recorder_reset(None) == 1
    assert lib.gcmx_record(None, None) == 1
    lib.gcmx_recorder_destroy(None)
    for name in ("recorder", "point_recorder", "record"):
        assert callable(getattr(gcm_amd.Context, name))


def test_task_settings_validate():
    from gcm_amd import _gcm_host as H
    t = H.Task()
    t.set_detector_buffer(0)
    t.set_detector_buffer(3)
    with pytest.raises(H.GcmException):
        t.set_detector_buffer(-1)
    t.set_receivers([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5]], ["Vx", "PRESSURE"])
    t.set_receivers([[1.0, 2.0]], ["Vy"], grid_id=1, buffer_steps=1)
    with pytest.raises(H.GcmException):
        t.set_receivers([], ["Vx"])
    with pytest.raises(H.GcmException):
        t.set_receivers([[1.0, 2.0, 3.0]], [])
    with pytest.raises(H.GcmException):
        t.set_receivers([[1.0, 2.0, 3.0]], ["Vx"] * 17)
    with pytest.raises(H.GcmException):
        t.set_receivers([[1.0, 2.0, 3.0]], ["Vx"], buffer_steps=0)
    with pytest.raises(H.GcmException):
        t.set_receivers([[1.0, float("nan"), 3.0]], ["Vx"])
    with pytest.raises(H.GcmException):
        t.set_receivers([[1.0, 2.0, 3.0, 4.0]], ["Vx"])
    with pytest.raises(Exception):
        t.set_receivers([[1.0, 2.0, 3.0]], ["no such quantity"])
    t.add_snapshotter("DETECTOR")
    with pytest.raises(H.GcmException):
        t.add_snapshotter("no such snapshotter")
