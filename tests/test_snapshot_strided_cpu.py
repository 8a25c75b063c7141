"""Strided snapshots without a GPU: the GPU-free VtkSnapshotter writer with
Task.set_vtk_stride / set_vtk_box against numpy, the ABI surface of
gcmx_snapshot_strided, and the writer's host code (host/snapshot.cpp) as a
stand-alone program under AddressSanitizer and UBSan
(tests/snapshot_strided_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import read_vts
from tests.taskspec import host_task, spec
from tests.test_abi import declared_symbols
from tests.test_observe_cpu import case_2d, case_3d, exact_layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


# ----------------------------------------------------------------- the writer --

def task_3d():
    """5 x 6 x 7 nodes from (2, -1, 4), h = (0.5, 0.25, 2), two materials."""
    s = spec(3, 2, [0.5, 0.25, 2.0], {0: ([5, 6, 7], [2, -1, 4])}, 0.9, (4, 2, 1), snaps=1)
    t = host_task(s)
    t.set_default_material(4, 2, 1, number=3)
    t.add_material(("box", (-1, -1, -1), (1.6, 100, 100)), 1, 1, 1, number=8)
    t.set_vtk_quantities(["Vz", "Syz", "PRESSURE"])
    return t, exact_layer((9, 10, 11, 9)), [5, 6, 7], [2, -1, 4], [0.5, 0.25, 2.0]


def task_2d():
    s = spec(2, 2, [0.5, 0.25], {0: ([9, 13], [3, -2])}, 0.9, (4, 2, 1), snaps=1,
             inhomogeneities=[(("box", (-10, -10, -10), (4.2, 100, 100)), (2, 1, 1))])
    t = host_task(s)
    t.set_vtk_quantities(["Sxy", "PRESSURE"])
    return t, exact_layer((13, 17, 5)), [9, 13], [3, -2], [0.5, 0.25]


SELECTIONS_3D = [([2, 3, 2], None), ([1, 1, 1], ([3, 0, 5], [6, 4, 10])), ([4, 7, 3], ([3, 0, 5], [100, 100, 100])),
                 ([2, 2, 5], ([-50, -50, -50], [4, 1, 9]))]
SELECTIONS_2D = [([2, 3], None), ([4, 5], ([4, 0], [11, 9])), ([1, 20], None)]


def local_selection(sizes, start, stride, box):
    lo = [0] * len(sizes) if box is None else [max(0, a - s) for a, s in zip(box[0], start)]
    hi = list(sizes) if box is None else [min(n, b - s) for n, b, s in zip(sizes, box[1], start)]
    return lo, hi, [slice(a, b, s) for a, b, s in zip(lo, hi, stride)]


@pytest.mark.parametrize("make,stride,box", [(task_3d, s, b) for s, b in SELECTIONS_3D] +
                         [(task_2d, s, b) for s, b in SELECTIONS_2D])
def test_strided_file_against_numpy(H, tmp_path, make, stride, box):
    t, layer, sizes, start, h = make()
    D = len(sizes)
    full = str(tmp_path / "full.vts")
    assert H.write_vtk(t, 0, full, layer) is True
    fdims, farrays, fpoints = read_vts(full)
    t.set_vtk_stride(stride)
    if box:
        t.set_vtk_box(*box)
    path = str(tmp_path / "sel.vts")
    assert H.write_vtk(t, 0, path, layer) is True
    dims, arrays, points = read_vts(path)
    lo, hi, sl = local_selection(sizes, start, stride, box)
    want_dims = [len(range(a, b, s)) for a, b, s in zip(lo, hi, stride)] + [1] * (3 - D)
    assert list(dims) == want_dims  # both extents are 0 ... n_d - 1
    text = open(path, "rb").read().split(b"<AppendedData")[0].decode()
    ext = " ".join(f"0 {n - 1}" for n in want_dims)
    assert f'WholeExtent="{ext}"' in text and f'Piece Extent="{ext}"' in text
    # Points: the float32 of the selected nodes' own coordinates, (real)start h + (real)it h
    its = np.meshgrid(*[np.arange(a, b, s) for a, b, s in zip(lo, hi, stride)], indexing="ij")
    coords = np.zeros(want_dims[::-1] + [3], np.float32)
    for d in range(D):
        c = np.float64(start[d]) * np.float64(h[d]) + its[d].astype(np.float64) * np.float64(h[d])
        coords[..., d] = np.transpose(c).astype(np.float32).reshape(want_dims[::-1])
    assert np.array_equal(points.view(np.uint32), coords.reshape(-1, 3).view(np.uint32))
    # every array, material_index included, is the full-resolution array at the selected nodes
    assert list(arrays) == list(farrays) and "material_index" in arrays and "Velocity" in arrays
    fshape = ([1] * (3 - D) + list(sizes)[::-1])
    vsl = tuple([slice(None)] * (3 - D) + sl[::-1])
    for name, a in arrays.items():
        want = farrays[name].reshape(fshape + [-1])[vsl].reshape(-1, a.shape[1])
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), name
    assert len(np.unique(arrays["material_index"])) >= 1
    # vtk_layer_arrays with the same selection gives the file's arrays
    qs = {3: ["Vz", "Syz", "PRESSURE"], 2: ["Sxy", "PRESSURE"]}[D]
    got = H.vtk_layer_arrays(sizes, 2, layer, qs, "elastic", lo, hi, stride)
    assert np.array_equal(got["Velocity"].view(np.uint32), arrays["Velocity"].view(np.uint32))
    assert np.array_equal(got["pressure"].view(np.uint32), arrays["pressure"][:, 0].view(np.uint32))


def test_materials_of_the_selected_nodes(H, tmp_path):
    """The 3-D task has two materials split along x: both show in the strided file, at their nodes."""
    t, layer, sizes, start, h = task_3d()
    t.set_vtk_stride([2, 5, 3])
    path = str(tmp_path / "m.vts")
    H.write_vtk(t, 0, path, layer)
    dims, arrays, points = read_vts(path)
    m = arrays["material_index"][:, 0]
    assert set(m) == {3.0, 8.0}
    assert np.array_equal(m == 8.0, points[:, 0] < 1.6)


@pytest.mark.parametrize("case", [case_2d, case_3d])
def test_stride_one_and_the_whole_box_is_the_existing_file(H, case, tmp_path):
    t, layer, name = case()
    args = (layer,) if layer is not None else ()
    old = str(tmp_path / "old.vts")
    H.write_vtk(t, 0, old, *args)
    D = t.dimensionality
    t.set_vtk_stride([1] * D)
    t.set_vtk_box([-1000] * D, [1000] * D)
    new = str(tmp_path / "new.vts")
    assert H.write_vtk(t, 0, new, *args) is True
    assert open(new, "rb").read() == open(old, "rb").read()
    assert open(new, "rb").read() == open(os.path.join(ROOT, "tests", "golden", name), "rb").read()


def test_a_body_the_box_misses_writes_no_file(H, tmp_path):
    t, layer, sizes, start, h = task_3d()
    t.set_vtk_box([7, -1, 4], [20, 5, 11])  # x from 7: the body ends at 2 + 5
    path = str(tmp_path / "none.vts")
    assert H.write_vtk(t, 0, path, layer) is False
    assert not os.path.exists(path)


def test_settings_are_refused_when_wrong(H):
    t = H.Task()
    for bad in ([0, 1, 1], [1, -2], [], [1, 1, 1, 1]):
        with pytest.raises(Exception):
            t.set_vtk_stride(bad)
    with pytest.raises(Exception):
        t.set_vtk_box([0, 0], [1, 1, 1])
    with pytest.raises(Exception):
        H.vtk_layer_arrays([5, 6, 7], 2, exact_layer((9, 10, 11, 9)), ["PRESSURE"], "elastic", [0, 0, 0], [5, 6, 8],
                           [1, 1, 1])
    with pytest.raises(Exception):
        H.vtk_layer_arrays([5, 6, 7], 2, exact_layer((9, 10, 11, 9)), ["PRESSURE"], "elastic", [0, 0, 0], [5, 6, 7],
                           [1, 0, 1])


# -------------------------------------------------------------------- the ABI --

def test_symbol_argtypes_and_abi_version():
    import gcm_amd
    from gcm_amd.gcmx import SYMBOLS
    assert "gcmx_snapshot_strided" in SYMBOLS
    assert sorted(SYMBOLS) == declared_symbols()
    lib = gcm_amd.lib()
    assert hasattr(lib, "gcmx_snapshot_strided")
    argtypes = lib.gcmx_snapshot_strided.argtypes
    assert argtypes is not None and len(argtypes) == 9
    assert lib.gcmx_abi_version() == 3
    assert "#define GCMX_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "gcmx.h")).read()
    assert callable(gcm_amd.Context.snapshot_strided)


def test_a_null_context_fails_loudly():
    import gcm_amd
    lib = gcm_amd.lib()
    qs = (ctypes.c_int * 1)(2)
    out_f = (ctypes.c_float * 12)()
    lo, hi, st = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(1, 1, 1), (ctypes.c_int * 3)(1, 1, 1)
    # the message of another failure first, so that an error without a message of its own is caught
    assert lib.gcmx_create(None, 0, None) != 0
    marker = lib.gcmx_last_error()
    assert lib.gcmx_snapshot_strided(None, lo, hi, st, 1, 1, qs, out_f, out_f) != 0
    msg = lib.gcmx_last_error()
    assert msg and msg != marker, msg
    assert not any(out_f)


# ------------------------------------------------------------ the sanitizers --

def test_writer_under_sanitizers(tmp_path):
    """host/snapshot.cpp and a main of its own, built with -fsanitize=address,undefined."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "snapshot_strided_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "snapshot_strided_check.cpp"),
                    os.path.join(ROOT, "gcm_amd", "host", "snapshot.cpp")], check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
