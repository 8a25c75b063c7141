"""Strided snapshots: gcmx_snapshot_strided (the STRIDED instance of k_pack_vtk,
k_pack_line with a stride) and the engine's VtkSnapshotter with
Task.set_vtk_stride / set_vtk_box on top of it.

Two forms of the expectation.  The first is ctx.snapshot_box of the same box
(held to the layer by tests/test_gpu_observe.py), sliced [::s] per axis in VTK
order.  The second does not go through the pack kernel at all: ctx.download()
pushed through getQuantityOf's formulas in numpy with the host's roundings, at
the selected nodes.  Every comparison is on the bit patterns."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers import context_for, oracle_body, random_state
from tests.taskspec import host_task, spec
from tests.test_gpu_observe import (ERR_INVALID_ARG, PRESSURE, acoustic_task, all_codes, f32, layer_of, quantity,
                                    random_context, same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


# ------------------------------------------------------------ expectations --

def lattice(lo, hi, st):
    return [-(-(b - a) // s) for a, b, s in zip(lo, hi, st)]


def sliced(ctx, lo, hi, st, codes, velocity=True):
    """ctx.snapshot_box of the box, every st[d]-th point per axis (VTK order: x fastest)."""
    vel, q = ctx.snapshot_box(lo, hi, codes, velocity=velocity)
    dims = [b - a for a, b in zip(lo, hi)][::-1]  # slowest first
    sl = tuple(slice(None, None, s) for s in list(st)[::-1])
    if velocity:
        vel = np.ascontiguousarray(vel.reshape(dims + [3])[sl]).reshape(-1, 3)
    n = int(np.prod(lattice(lo, hi, st)))
    q = np.ascontiguousarray(q.reshape([len(codes)] + dims)[(slice(None),) + sl]).reshape(len(codes), n)
    return vel, q


def from_layer(ctx, layer, lo, hi, st, codes):
    """The values formed from the downloaded layer with the host's roundings."""
    D, M, bs = ctx.dim, ctx.M, ctx.bs
    box = layer[tuple(slice(bs + a, bs + b, s) for a, b, s in zip(lo, hi, st))]
    rows = np.transpose(box, tuple(range(D - 1, -1, -1)) + (D,)).reshape(-1, M)  # x fastest
    vel = np.zeros((len(rows), 3), np.float32)
    vel[:, :D] = f32(rows[:, :D])
    q = np.stack([f32(quantity(ctx.model, D, M, c, rows)) for c in codes])
    return vel, q


def check(ctx, lo, hi, st, codes=None, independent=False, layer=None):
    codes = all_codes(ctx.model, ctx.dim, ctx.M) if codes is None else codes
    n = int(np.prod(lattice(lo, hi, st)))
    if independent and layer is None:
        layer = layer_of(ctx)
    for part in (codes[:16], codes[16:]):  # GCMX_MAX_BORDER_Q per call
        if not part:
            continue
        vel, q = ctx.snapshot_strided(lo, hi, st, part)
        assert vel.shape == (n, 3) and q.shape == (len(part), n), (vel.shape, q.shape, n)
        wv, wq = sliced(ctx, lo, hi, st, part)
        same_bits(vel, wv, f"Velocity {ctx.sizes} {lo} {hi} {st}")
        same_bits(q, wq, f"quantities {part} {ctx.sizes} {lo} {hi} {st}")
        if independent:
            wv, wq = from_layer(ctx, layer, lo, hi, st, part)
            same_bits(vel, wv, f"Velocity against the layer {ctx.sizes} {lo} {hi} {st}")
            same_bits(q, wq, f"quantities against the layer {part} {ctx.sizes} {lo} {hi} {st}")
    if ctx.dim < 3:
        assert not vel[:, ctx.dim:].view(np.uint32).any()  # +0.0f padding
    none, q = ctx.snapshot_strided(lo, hi, st, codes[:3], velocity=False)
    assert none is None
    same_bits(q, sliced(ctx, lo, hi, st, codes[:3])[1], f"velocity=False {ctx.sizes} {st}")
    vel, q = ctx.snapshot_strided(lo, hi, st, [])
    assert q.shape == (0, n)
    same_bits(vel, sliced(ctx, lo, hi, st, [])[0], f"Velocity alone {ctx.sizes} {st}")


# ------------------------------------------------------------- the lattice --

CASES = [
    ([5, 7, 70], None, None, (1, 1, 1)),       # equals snapshot_box
    ([130, 3, 5], None, None, (2, 1, 1)),      # 65 output A: two tiles along A
    ([3, 2, 195], None, None, (1, 1, 3)),      # 65 output F: two tiles along F
    ([9, 9, 9], None, None, (4, 4, 4)),        # extent not a multiple of the stride; 3 points per axis
    ([6, 5, 7], None, None, (7, 9, 8)),        # one point per axis
    ([12, 10, 140], [1, 2, 3], [11, 9, 137], (3, 2, 5)),  # odd minimum, unaligned rows
    ([70, 131], None, None, (3, 2)),
    ([131, 9], None, None, (2, 4)),
    ([40], None, None, (7,)),
    # one load method at every stride (no switch): 65 output F at 4, 5 and 16 (a lane per 128-byte line)
    ([3, 2, 64 * 4 + 2], None, None, (1, 1, 4)),
    ([3, 2, 64 * 5 + 2], None, None, (1, 1, 5)),
    ([2, 2, 64 * 16 + 2], None, None, (1, 1, 16)),
    ([2, 70 * 2], None, None, (1, 2)),         # 2-D, two tiles along F
    ([2, 66 * 9], None, None, (1, 9)),
]


@pytest.mark.parametrize("sizes,lo,hi,st", CASES, ids=[f"{c[0]}-{c[3]}" for c in CASES])
def test_lattice(G, sizes, lo, hi, st):
    ctx = random_context(G, sizes)
    lo = [0] * len(sizes) if lo is None else lo
    hi = list(sizes) if hi is None else hi
    check(ctx, lo, hi, st, independent=True)
    ctx.close()


def test_unit_stride_is_snapshot_box(G):
    ctx = random_context(G, [5, 7, 70])
    codes = [PRESSURE, 64 + 4, 4]
    for lo, hi in (([0, 0, 0], [5, 7, 70]), ([1, 2, 3], [4, 6, 69])):
        v0, q0 = ctx.snapshot_box(lo, hi, codes)
        v1, q1 = ctx.snapshot_strided(lo, hi, [1, 1, 1], codes)
        same_bits(v1, v0, "Velocity, stride 1")
        same_bits(q1, q0, "quantities, stride 1")
    ctx.close()


def test_stride_beyond_the_extent_is_one_point(G):
    ctx = random_context(G, [6, 5, 7])
    layer = layer_of(ctx)
    big = 2 ** 31 - 1
    for st in ((big, big, big), (6, 5, 7), (1, big, 1), (big, 1, 2)):
        check(ctx, [0, 0, 0], [6, 5, 7], st, [PRESSURE, 64 + 8], independent=True, layer=layer)
        check(ctx, [2, 1, 3], [6, 4, 7], st, [PRESSURE, 64 + 8], independent=True, layer=layer)
    ctx.close()


@pytest.mark.parametrize("bs", [1, 2, 3])
def test_border_sizes(G, bs):
    ctx = random_context(G, [9, 7, 70], bs)
    check(ctx, [0, 0, 0], [9, 7, 70], (2, 3, 3), independent=True)
    check(ctx, [1, 0, 2], [9, 6, 69], (3, 2, 7), [PRESSURE, 64 + 8, 2], independent=True)
    ctx.close()


@pytest.mark.parametrize("sizes,st", [([5, 6, 70], (2, 2, 3)), ([15, 70], (2, 3)), ([15, 70], (4, 7))])
def test_acoustic(G, sizes, st):
    ctx = random_context(G, sizes, 2, model="acoustic")
    assert ctx.M == len(sizes) + 1
    check(ctx, [0] * len(sizes), sizes, st, independent=True)
    with pytest.raises(G.GcmxError) as e:
        ctx.snapshot_strided([0] * len(sizes), sizes, st, [5])  # Sxx: not in the acoustic vector
    assert e.value.status == ERR_INVALID_ARG
    ctx.close()


@pytest.mark.parametrize("pads", [{"GCMX_ROW_PAD": "1"}, {"GCMX_PLANE_PAD": "3"}, {"GCMX_CS_PAD": "5"},
                                  {"GCMX_ROW_PAD": "1", "GCMX_PLANE_PAD": "3", "GCMX_CS_PAD": "5"}])
def test_padded_layout(G, monkeypatch, pads):
    """Every stride of the layer comes from the context's geometry, none from the sizes."""
    plain = G.Context(3, 2, [5, 7, 70])
    plain_geo = plain.geometry()
    plain.close()
    for k, v in pads.items():
        monkeypatch.setenv(k, v)
    ctx = random_context(G, [5, 7, 70])
    geo = ctx.geometry()
    assert (geo["stride"], geo["cs"]) != (plain_geo["stride"], plain_geo["cs"]), (geo, plain_geo)
    for st in ((2, 3, 3), (1, 2, 6)):
        check(ctx, [0, 0, 0], [5, 7, 70], st, [PRESSURE, 64 + 8, 2], independent=True)
    check(ctx, [1, 1, 1], [5, 6, 70], (3, 2, 2), [PRESSURE, 64 + 8, 2], independent=True)
    ctx.close()
    ctx2 = random_context(G, [9, 70])
    check(ctx2, [0, 0], [9, 70], (2, 3), independent=True)
    ctx2.close()


def test_structured_state_names_its_node(G):
    """Every component of a node holds that node's global index (all nodes, ghosts
    included), exactly representable in Float32: a wrong node shows as a wrong
    integer."""
    for sizes, lo, hi, st in (([12, 10, 140], [1, 2, 3], [11, 9, 137], (3, 2, 5)),
                              ([12, 10, 140], [0, 0, 0], [12, 10, 140], (5, 3, 2)),
                              ([70, 131], [1, 0], [70, 130], (3, 7)), ([40], [3], [38], (4,))):
        D, bs = len(sizes), 2
        M = G.gcmx.pde_size(D)
        shape_all = [s + 2 * bs for s in sizes]
        n_all = int(np.prod(shape_all))
        assert n_all < 2 ** 24
        state = np.repeat(np.arange(n_all, dtype=np.float64)[:, None], M, axis=1)
        ctx = G.Context(D, bs, sizes)
        ctx.upload(state)
        comps = [64 + c for c in range(M)]
        vel, q = ctx.snapshot_strided(lo, hi, st, comps)
        idx = np.arange(n_all).reshape(shape_all)[tuple(slice(bs + a, bs + b, s) for a, b, s in zip(lo, hi, st))]
        want = np.transpose(idx, tuple(range(D - 1, -1, -1))).reshape(-1).astype(np.float32)
        for c in range(M):
            assert np.array_equal(q[c], want), (sizes, st, c, q[c][:8], want[:8])
        for c in range(D):
            assert np.array_equal(vel[:, c], want), (sizes, st, c)
        ctx.close()


# ---------------------------------------------------------------- refusals --

MARK = np.float32(-12345.5)


def raw_call(G, ctx, lo, hi, st, want_velocity, codes, vel, out):
    ip = lambda v: None if v is None else (ctypes.c_int * 3)(*(list(v) + [0] * (3 - len(v))))
    fp = ctypes.POINTER(ctypes.c_float)
    q = (ctypes.c_int * max(1, len(codes)))(*codes)
    return G.lib().gcmx_snapshot_strided(ctx.ptr, ip(lo), ip(hi), ip(st), want_velocity, len(codes), q,
                                         None if vel is None else vel.ctypes.data_as(fp),
                                         None if out is None else out.ctypes.data_as(fp))


def test_refusals(G):
    ctx = random_context(G, [4, 5, 6])
    box = ([0, 0, 0], [4, 5, 6])
    one = [1, 1, 1]
    bad = [
        (box[0], box[1], [0, 1, 1], 1, [2]), (box[0], box[1], [1, -1, 1], 1, [2]), (box[0], box[1], [1, 1, 0], 1, [2]),
        (box[0], box[1], None, 1, [2]),                                  # a null stride
        (None, box[1], one, 1, [2]), (box[0], None, one, 1, [2]),        # a null box
        ([2, 0, 0], [2, 5, 6], one, 1, [2]), ([0, 3, 0], [4, 2, 6], [2, 2, 2], 1, [2]),  # empty
        ([0, 0, 0], [4, 5, 7], [2, 2, 2], 1, [2]), ([-1, 0, 0], [4, 5, 6], [2, 2, 2], 1, [2]),  # outside
        (box[0], box[1], [2, 2, 2], 0, []),                              # nothing asked for
        (box[0], box[1], [2, 2, 2], 1, [13]), (box[0], box[1], [2, 2, 2], 1, [64 + 9]),
        (box[0], box[1], [2, 2, 2], 1, [2] * 17),
    ]
    before = ctx.transfer_bytes()
    layer = ctx.download()
    at = ctx.transfer_bytes()
    for lo, hi, st, wv, codes in bad:
        vel = np.full((120, 3), MARK)
        out = np.full((17, 120), MARK)
        assert G.lib().gcmx_create(None, 0, None) != 0  # the message of another failure first
        marker = G.lib().gcmx_last_error()
        status = raw_call(G, ctx, lo, hi, st, wv, codes, vel, out)
        assert status == ERR_INVALID_ARG, (lo, hi, st, codes, status)
        msg = G.lib().gcmx_last_error()
        assert msg and msg != marker, (lo, hi, st, codes, msg)
        assert (vel == MARK).all() and (out == MARK).all(), (lo, hi, st, codes)
    # a null buffer that is asked for
    vel = np.full((120, 3), MARK)
    out = np.full((1, 120), MARK)
    assert raw_call(G, ctx, box[0], box[1], [2, 2, 2], 1, [2], None, out) == ERR_INVALID_ARG
    assert G.lib().gcmx_last_error()
    assert raw_call(G, ctx, box[0], box[1], [2, 2, 2], 1, [2], vel, None) == ERR_INVALID_ARG
    assert raw_call(G, ctx, box[0], box[1], [2, 2, 2], 0, [2], None, None) == ERR_INVALID_ARG
    assert (vel == MARK).all() and (out == MARK).all()
    # ... and one that is not asked for may be null
    assert raw_call(G, ctx, box[0], box[1], [2, 2, 2], 0, [2], None, out) == 0
    assert (out[0, :18] != MARK).all() and (out[0, 18:] == MARK).all()  # 2 x 3 x 3 points, no more
    # the Python wrapper raises, and nothing was copied or changed by a refused call
    with pytest.raises(G.GcmxError) as e:
        ctx.snapshot_strided(box[0], box[1], [0, 1, 1], [2])
    assert e.value.status == ERR_INVALID_ARG
    assert ctx.transfer_bytes()[0] == at[0] + 18 * 4 and ctx.transfer_bytes()[1] == before[1]
    assert np.array_equal(ctx.download().view(np.uint64), layer.view(np.uint64))
    ctx2 = random_context(G, [4, 9])
    with pytest.raises(G.GcmxError):
        ctx2.snapshot_strided([0, 0], [4, 9], [2, 2], [4])  # Vz in 2-D
    # entries >= dim of the box and the stride are ignored
    out = np.full((1, 10), MARK)
    assert raw_call(G, ctx2, [0, 0, 5], [4, 9, 3], [2, 2, -7], 0, [PRESSURE], None, out) == 0
    same_bits(out, sliced(ctx2, [0, 0], [4, 9], [2, 2], [PRESSURE], velocity=False)[1], "entries >= dim ignored")
    ctx.close()
    ctx2.close()


# ------------------------------------------------------ transfer accounting --

@pytest.mark.parametrize("want_velocity,codes", [(True, [PRESSURE]), (True, []), (False, [PRESSURE, 2, 64 + 8]),
                                                 (True, [2, 3, 4, PRESSURE])])
def test_transfer_bytes_are_the_output(G, want_velocity, codes):
    ctx = random_context(G, [9, 8, 75])
    for lo, hi, st in (([0, 0, 0], [9, 8, 75], (2, 3, 4)), ([1, 2, 3], [8, 5, 71], (1, 2, 9)),
                       ([0, 0, 0], [9, 8, 75], (1, 1, 1))):
        n = int(np.prod(lattice(lo, hi, st)))
        at = ctx.transfer_bytes()
        ctx.snapshot_strided(lo, hi, st, codes, velocity=want_velocity)
        now = ctx.transfer_bytes()
        assert now[0] - at[0] == n * 4 * (3 * want_velocity + len(codes)), (lo, hi, st)
        assert now[1] == at[1]
    ctx.close()


def test_separate_buffers_take_two_copies_of_the_same_bytes(G):
    ctx = random_context(G, [9, 8, 75])
    lo, hi, st = [0, 0, 0], [9, 8, 75], [2, 3, 4]
    n = int(np.prod(lattice(lo, hi, st)))
    vel = np.full((n + 5, 3), MARK)
    out = np.full((2, n), MARK)
    at = ctx.transfer_bytes()[0]
    assert raw_call(G, ctx, lo, hi, st, 1, [PRESSURE, 3], vel, out) == 0
    assert ctx.transfer_bytes()[0] - at == n * 4 * 5
    wv, wq = sliced(ctx, lo, hi, st, [PRESSURE, 3])
    same_bits(vel[:n], wv, "Velocity, separate buffers")
    same_bits(out, wq, "quantities, separate buffers")
    assert (vel[n:] == MARK).all()
    ctx.close()


def test_the_call_changes_no_state(G):
    sizes = [6, 9, 37]
    b = oracle_body(3, 2, sizes)
    random_state(b, 5, ghosts=False)
    seen, twin = context_for(b), context_for(b)
    tau = 0.9 / b.maximal_eigenvalue
    path = seen.effective_path
    assert path == twin.effective_path == "fused"
    for _ in range(2):
        seen.snapshot_strided([0, 0, 0], sizes, [2, 2, 3], [PRESSURE])
        seen.snapshot_strided([1, 0, 2], sizes, [1, 4, 7], [PRESSURE, 2])
        assert seen.effective_path == path
        a, c = seen.download(), twin.download()
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64))
        seen.step(tau)
        twin.step(tau)
        assert seen.last_path == twin.last_path == "fused"
        a, c = seen.download(), twin.download()
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64))
    seen.close()
    twin.close()


# ------------------------------------------------------------------ engine --

def read(path):
    with open(path, "rb") as f:
        return f.read()


def run_and_compare(H, make_task, bodies, steps_per_snap, tmp_path, monkeypatch, chunk=None):
    """Run the task with the VTK snapshotter; a twin engine's layers (pdeAll) go
    through the GPU-free writer with the same selection: the files must be equal
    byte for byte, a body the box misses has none.  Returns (engine, snapshots,
    {body: selected points})."""
    monkeypatch.chdir(tmp_path)
    t = make_task()
    t.add_snapshotter("VTK")
    t.output_directory = "seen"
    if chunk:
        t.set_vtk_chunk_bytes(chunk)
    he = H.Engine(t)
    he.run()
    twin = H.Engine(make_task())
    snaps, points = 0, {}
    for step in range(he.steps + 1):
        if step:
            twin.run_steps(1)
        if step % steps_per_snap:
            continue
        snaps += 1
        for i in bodies:
            got = f"snapshots/seen/vtk/mesh{i}core00snap{step:04d}.vts"
            want = f"want/{i}_{step}.vts"
            if H.write_vtk(t, i, want, twin.pde(i)):
                assert read(got) == read(want), (i, step)
                from tests.helpers import read_vts
                dims, _, _ = read_vts(got)
                points[i] = int(np.prod(dims))
            else:
                assert not os.path.exists(got) and not os.path.exists(want), (i, step)
                points[i] = 0
    return he, snaps, points


def body_task(stride, box):
    def make():
        s = spec(3, 2, [1, 1, 1], {0: ([20, 12, 18], [0, 0, 0])}, 0.9, (4, 2, 1), snaps=2, steps_per_snap=2,
                 quantities=[(("sphere", 4.0, (10.0, 6.0, 9.0)), "PRESSURE", 10.0)])
        t = host_task(s)
        t.set_vtk_quantities(["PRESSURE", "Vz"])
        if stride:
            t.set_vtk_stride(stride)
        if box:
            t.set_vtk_box(*box)
        return t
    return make


@pytest.mark.parametrize("stride,box,n,chunk", [
    ([2, 3, 2], None, 10 * 4 * 9, None),
    ([2, 3, 2], ([3, 1, 2], [19, 12, 17]), 8 * 4 * 8, None),
    ([2, 3, 2], ([3, 1, 2], [19, 12, 17]), 8 * 4 * 8, 8 * 4 * 20 * 3),  # slabs of three output planes
    (None, ([3, 1, 2], [1000, 1000, 17]), 17 * 11 * 15, 1024),          # a box alone, clipped to the body
])
def test_engine_body(H, tmp_path, monkeypatch, stride, box, n, chunk):
    he, snaps, points = run_and_compare(H, body_task(stride, box), [0], 2, tmp_path, monkeypatch, chunk)
    assert snaps == 3 and points == {0: n}
    # the run's device-to-host bytes are those of the selected points: Velocity + two quantities
    assert he.transfer_bytes(0)[0] == snaps * n * 4 * 5


def stack_task(stride, box):
    def make():
        X, Z = 10, 64
        cubics = {0: ([X, 5, Z], [0, 0, 0]), 1: ([X, 7, Z], [0, 5, 0])}
        s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=2, steps_per_snap=2,
                 quantities=[(("sphere", 5.0, (X / 2, 3.5, Z / 2)), "PRESSURE", 10.0)])
        t = host_task(s)
        t.set_vtk_quantities(["PRESSURE", "Vy"])
        t.set_vtk_stride(stride)
        if box:
            t.set_vtk_box(*box)
        return t
    return make


def test_engine_stack_members(H, tmp_path, monkeypatch):
    """Two members of a y stack: each selects from its own nodes, at its own offset
    in the stack's context; the box is clipped to each."""
    he, snaps, points = run_and_compare(H, stack_task([2, 3, 2], ([1, 2, 3], [9, 11, 60])), [0, 1], 2, tmp_path,
                                        monkeypatch)
    assert he.last_path(0) == "fused" and he.last_path(1) == "fused"
    # member 0: y 2..4 -> 1 point; member 1: y 5..10 -> local 0..5 -> 2 points
    assert points == {0: 4 * 1 * 29, 1: 4 * 2 * 29}
    d2h = he.transfer_bytes(0)[0]
    assert d2h == he.transfer_bytes(1)[0]  # one context behind both members
    assert d2h == snaps * (points[0] + points[1]) * 4 * 5


def test_engine_body_outside_the_box_writes_no_file(H, tmp_path, monkeypatch):
    he, snaps, points = run_and_compare(H, stack_task([2, 3, 2], ([0, 6, 0], [10, 12, 64])), [0, 1], 2, tmp_path,
                                        monkeypatch)
    assert points == {0: 0, 1: 5 * 2 * 32}
    assert he.transfer_bytes(0)[0] == snaps * points[1] * 4 * 5


def test_engine_acoustic_2d(H, tmp_path, monkeypatch):
    def make():
        t = acoustic_task(H)
        t.set_vtk_stride([3, 2])
        t.set_vtk_box([2, 1], [39, 30])
        return t
    he, snaps, points = run_and_compare(H, make, [0], 2, tmp_path, monkeypatch)
    assert he.matrix_structure(0) == 3
    assert points == {0: 13 * 15}
    assert he.transfer_bytes(0)[0] == snaps * 13 * 15 * 4 * 5
