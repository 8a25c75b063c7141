"""Observation without whole-layer downloads: gcmx_snapshot_box (k_pack_vtk),
gcmx_gather (k_gather_q), gcmx_scan (k_scan), gcmx_transfer_stats, and the
engine's snapshotters on top of them.

Expected values never come from the code under test: they are ctx.download()
(held to the oracle by the parity suites) pushed through getQuantityOf's formulas
in numpy (host/task.hpp:134-143, host/acoustic_model.hpp:145-180) and numpy's
float64 -> float32 conversion (round to nearest even).  Every comparison is on
the bit patterns."""
import numpy as np
import pytest

from tests.helpers import context_for, oracle_body, random_state
from tests.taskspec import host_task, spec

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = 1
PRESSURE = 12


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

def sigma(D, i, j):
    return D + i * D - ((i - 1) * i) // 2 + j - i


def quantity(model, D, M, code, v):
    """getQuantityOf on rows v [n, M], in float64 with the host's roundings."""
    if code >= 64:
        return v[:, code - 64]
    if code in (2, 3, 4):
        return v[:, code - 2]
    if model == "acoustic":
        assert code == PRESSURE
        return v[:, D]
    if code == PRESSURE:
        trace = np.zeros(len(v))
        for d in range(D):
            trace = trace + v[:, sigma(D, d, d)]
        return -trace / float(D)
    ij = {5: (0, 0), 6: (0, 1), 7: (0, 2), 8: (1, 1), 9: (1, 2), 10: (2, 2)}[code]
    return v[:, sigma(D, *ij)]


def all_codes(model, D, M):
    """Every component by GCMX_Q_COMPONENT, every named quantity the vector has, PRESSURE."""
    named = [2 + d for d in range(D)]
    if model == "elastic":
        named += [c for c, (i, j) in {5: (0, 0), 6: (0, 1), 7: (0, 2), 8: (1, 1), 9: (1, 2),
                                      10: (2, 2)}.items() if i < D and j < D]
    return [64 + c for c in range(M)] + named + [PRESSURE]


def f32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def layer_of(ctx):
    return ctx.download().reshape(ctx.shape_all + (ctx.M,))


def expected_box(ctx, layer, lo, hi, codes):
    D, M, bs = ctx.dim, ctx.M, ctx.bs
    box = layer[tuple(slice(bs + a, bs + b) for a, b in zip(lo, hi))]
    rows = np.transpose(box, tuple(range(D - 1, -1, -1)) + (D,)).reshape(-1, M)  # x fastest
    vel = np.zeros((len(rows), 3), np.float32)
    vel[:, :D] = f32(rows[:, :D])
    q = np.stack([f32(quantity(ctx.model, D, M, c, rows)) for c in codes]) if codes else np.zeros((0, len(rows)), np.float32)
    return vel, q


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = got.view(u) != want.view(u)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} differ; first at "
                           f"{tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r} "
                           f"want {want[tuple(np.argwhere(bad)[0])]!r}")


def random_context(G, sizes, bs=2, model="elastic", seed=None):
    """A context whose whole layer, ghosts included, is random (what
    helpers.random_state(..., ghosts=True) gives a body): a read outside the box
    would show.  The observation calls need no materials."""
    D = len(sizes)
    M = G.gcmx.pde_size(D, model)
    rng = np.random.default_rng(sum(sizes) + bs if seed is None else seed)
    state = rng.uniform(-1, 1, (int(np.prod([s + 2 * bs for s in sizes])), M))
    ctx = G.Context(D, bs, sizes, model=model)
    ctx.upload(state)
    return ctx


def check_whole_box(ctx, codes=None):
    D = ctx.dim
    codes = all_codes(ctx.model, D, ctx.M) if codes is None else codes
    layer = layer_of(ctx)
    lo, hi = [0] * D, list(ctx.sizes)
    for part in (codes[:16], codes[16:]):  # GCMX_MAX_BORDER_Q per call
        if not part:
            continue
        vel, q = ctx.snapshot_box(lo, hi, part)
        wv, wq = expected_box(ctx, layer, lo, hi, part)
        same_bits(vel, wv, f"Velocity {ctx.sizes}")
        same_bits(q, wq, f"quantities {part} {ctx.sizes}")
    if D < 3:
        assert not vel[:, D:].view(np.uint32).any()  # +0.0f padding
    none, q = ctx.snapshot_box(lo, hi, codes[:3], velocity=False)
    assert none is None
    same_bits(q, expected_box(ctx, layer, lo, hi, codes[:3])[1], f"velocity=False {ctx.sizes}")
    vel, q = ctx.snapshot_box(lo, hi, [])
    assert q.shape == (0, len(vel))
    same_bits(vel, expected_box(ctx, layer, lo, hi, [])[0], f"Velocity alone {ctx.sizes}")


# ------------------------------------------------------------ snapshot_box --

@pytest.mark.parametrize("sizes", [[5, 7, 70], [66, 3, 5], [65, 2, 65], [1, 1, 4], [70, 9], [9, 70], [40]])
def test_snapshot_box_whole_inner_box(G, sizes):
    bs = 1 if sizes == [1, 1, 4] else 2
    ctx = random_context(G, sizes, bs)
    before = ctx.transfer_bytes()
    check_whole_box(ctx)
    # one call moves exactly its output: Velocity and one quantity, 16 bytes per node
    at = ctx.transfer_bytes()
    ctx.snapshot_box([0] * len(sizes), sizes, [PRESSURE])
    assert ctx.transfer_bytes()[0] - at[0] == 16 * int(np.prod(sizes))
    assert ctx.transfer_bytes()[1] == before[1]
    ctx.close()


@pytest.mark.parametrize("bs", [1, 2, 3])
def test_snapshot_box_border_sizes(G, bs):
    ctx = random_context(G, [5, 7, 70], bs)
    check_whole_box(ctx)
    ctx.close()


@pytest.mark.parametrize("sizes", [[5, 6, 70], [15, 11]])
def test_snapshot_box_acoustic(G, sizes):
    ctx = random_context(G, sizes, 2, model="acoustic")
    assert ctx.M == len(sizes) + 1
    check_whole_box(ctx)
    with pytest.raises(G.GcmxError) as e:
        ctx.snapshot_box([0] * len(sizes), sizes, [5])  # Sxx: not in the acoustic vector
    assert e.value.status == ERR_INVALID_ARG
    ctx.close()


def test_snapshot_box_sub_boxes(G):
    sizes = [9, 8, 75]
    ctx = random_context(G, sizes)
    layer = layer_of(ctx)
    codes = [PRESSURE, 64 + 4, 4]
    for lo, hi in (([1, 2, 3], [8, 5, 71]), ([1, 2, 3], [9, 8, 75]), ([1, 2, 3], [2, 3, 4]),
                   ([0, 0, 64], [9, 8, 65])):
        vel, q = ctx.snapshot_box(lo, hi, codes)
        wv, wq = expected_box(ctx, layer, lo, hi, codes)
        same_bits(vel, wv, f"Velocity {lo} {hi}")
        same_bits(q, wq, f"quantities {lo} {hi}")
    # two z slabs concatenated are the whole box (z is the slowest VTK axis)
    whole_v, whole_q = ctx.snapshot_box([0, 0, 0], sizes, codes)
    v0, q0 = ctx.snapshot_box([0, 0, 0], [9, 8, 31], codes)
    v1, q1 = ctx.snapshot_box([0, 0, 31], sizes, codes)
    same_bits(np.concatenate([v0, v1]), whole_v, "slabs, Velocity")
    same_bits(np.concatenate([q0, q1], axis=1), whole_q, "slabs, quantities")
    ctx.close()


def test_snapshot_box_refusals(G):
    ctx = random_context(G, [4, 5, 6])
    bad = [(([0, 0, 0], [4, 5, 7]), [2]), (([-1, 0, 0], [4, 5, 6]), [2]), (([2, 0, 0], [2, 5, 6]), [2]),
           (([0, 3, 0], [4, 2, 6]), [2]), (([0, 0, 0], [4, 5, 6]), [13]), (([0, 0, 0], [4, 5, 6]), [64 + 9]),
           (([0, 0, 0], [4, 5, 6]), [2] * 17)]
    for (lo, hi), codes in bad:
        with pytest.raises(G.GcmxError) as e:
            ctx.snapshot_box(lo, hi, codes)
        assert e.value.status == ERR_INVALID_ARG, (lo, hi, codes)
    with pytest.raises(G.GcmxError) as e:  # nothing asked for
        ctx.snapshot_box([0, 0, 0], [4, 5, 6], [], velocity=False)
    assert e.value.status == ERR_INVALID_ARG
    import ctypes
    lo, hi, q = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 5, 6), (ctypes.c_int * 1)(2)
    assert G.lib().gcmx_snapshot_box(ctx.ptr, lo, hi, 1, 1, q, None, None) == ERR_INVALID_ARG  # null outputs
    ctx2 = random_context(G, [4, 9], model="elastic")
    with pytest.raises(G.GcmxError):
        ctx2.snapshot_box([0, 0], [4, 9], [4])  # Vz in 2-D
    with pytest.raises(G.GcmxError):
        ctx2.snapshot_box([0, 0], [4, 9], [7])  # Sxz in 2-D
    ctx.close()
    ctx2.close()


@pytest.mark.parametrize("pads", [{"GCMX_ROW_PAD": "1"}, {"GCMX_PLANE_PAD": "3"},
                                  {"GCMX_ROW_PAD": "1", "GCMX_PLANE_PAD": "1"}])
def test_padded_layout(G, monkeypatch, pads):
    """Rows and planes that start at odd elements: every stride comes from the
    context's geometry, none from the sizes."""
    for k, v in pads.items():
        monkeypatch.setenv(k, v)
    ctx = random_context(G, [5, 7, 70])
    geo = ctx.geometry()
    assert geo["row"] % 2 == 1 or geo["stride"][0] % 2 == 1, geo
    check_whole_box(ctx, [PRESSURE, 64 + 8, 2])
    nodes = np.array([[4, 6, 69], [0, 0, 0], [2, 3, 64]])
    nl = ctx.node_list(nodes)
    layer = layer_of(ctx)
    rows = layer[nodes[:, 0] + 2, nodes[:, 1] + 2, nodes[:, 2] + 2]
    same_bits(ctx.gather(nl, [PRESSURE, 64 + 5]),
              np.stack([quantity("elastic", 3, 9, c, rows) for c in (PRESSURE, 64 + 5)]), "gather, padded")
    bad, mx = ctx.scan()
    inner = layer[2:-2, 2:-2, 2:-2].reshape(-1, 9)
    assert bad == 0
    same_bits(mx, np.abs(inner).max(axis=0), "scan, padded")
    ctx.close()


def test_structured_values(G):
    """Signs of zero through the trace, Float32 overflow and underflow, ties to even,
    and an inexact division by three, all in one state."""
    sizes = [3, 4, 16]
    b = oracle_body(3, 2, sizes)
    random_state(b, 3, ghosts=True)
    inner = b.inner_view()
    e24 = 2.0 ** -24
    specials = [
        # (velocity x3, Sxx, Sxy, Sxz, Syy, Syz, Szz)
        [0.0, -0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0],      # +0 trace -> PRESSURE -0.0
        [-0.0, 0.0, -0.0, -0.0, 1.0, 1.0, -0.0, 1.0, -0.0],  # 0.0 + -0.0 = +0.0 -> -0.0 again
        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.0, 0.0, 0.0],
        [1e300, -1e300, 1e300, 1e300, -1e300, 1.0, 1e300, 1.0, 1e300],     # -> +-inf
        [-1e300, 1e300, -1e300, -1e300, 1e300, 1.0, -1e300, 1.0, -1e300],
        [1e-320, -1e-320, 1e-46, 1e-320, -1e-320, 1e-46, 1e-320, -1e-46, 1e-320],  # -> +-0
        [-1e-46, 1e-46, -1e-320, -1e-46, 1e-46, -1e-320, -1e-46, 1e-46, -1e-46],
        [1 + e24, 1 + 3 * e24, -(1 + e24), 1 + e24, -(1 + 3 * e24), 1.0, 1 + 3 * e24, 1.0, 1 + e24],  # ties
        [0.1, 0.2, 0.3, 0.25, 0.0, 0.0, 0.25, 0.0, 0.5],     # trace 1.0: -1/3 is inexact
        [0.1, 0.2, 0.3, 0.1, 0.0, 0.0, 0.2, 0.0, 0.3],       # inexact sums, inexact division
    ]
    for k, row in enumerate(specials):
        inner[1, 2, k] = row
        inner[2, 1, 15 - k] = row[::-1]
    ctx = G.Context(3, 2, sizes)
    ctx.upload(b.pde)
    layer = layer_of(ctx)
    assert np.array_equal(layer.view(np.uint64), b.pde.reshape(layer.shape).view(np.uint64))
    codes = all_codes("elastic", 3, 9)
    check_whole_box(ctx, codes)
    # the expectation itself holds the cases it is meant to
    _, q = expected_box(ctx, layer, [1, 2, 0], [2, 3, 16], [PRESSURE, 64, 64 + 3])
    p = q[0]
    assert p[0] == 0 and np.signbit(p[0]) and np.signbit(p[1]) and np.signbit(p[2])
    assert np.isinf(p[3]) and p[3] < 0 and np.isinf(p[4]) and p[4] > 0
    assert np.isinf(q[1][3]) and q[1][5] == 0 and not np.signbit(q[1][5]) and np.signbit(q[1][6])
    assert q[1][7] == np.float32(1.0) and q[2][7] == np.float32(1.0)
    assert f32([1 + 3 * e24])[0] == np.float32(1 + 4 * e24)
    assert float(p[8]) != -1.0 / 3.0 and p[8] == np.float32(-1.0 / 3.0)
    nodes = np.array([[1, 2, k] for k in range(16)] + [[2, 1, k] for k in range(16)])
    nl = ctx.node_list(nodes)
    rows = layer[nodes[:, 0] + 2, nodes[:, 1] + 2, nodes[:, 2] + 2]
    got = ctx.gather(nl, codes[:16])
    same_bits(got, np.stack([quantity("elastic", 3, 9, c, rows) for c in codes[:16]]), "gather, structured")
    ctx.close()


# ------------------------------------------------------------------ gather --

@pytest.fixture(scope="module")
def gather_ctx(G):
    ctx = random_context(G, [6, 9, 37])
    yield ctx, layer_of(ctx)
    ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_gather(G, gather_ctx, n):
    ctx, layer = gather_ctx
    rng = np.random.default_rng(n)
    nodes = np.stack([rng.integers(0, s, n) for s in ctx.sizes], axis=1)  # shuffled, repeats for n = 1000
    if n >= 63:
        nodes[5] = nodes[17]
        assert len(np.unique(nodes, axis=0)) < n
    nl = ctx.node_list(nodes)
    rows = layer[nodes[:, 0] + 2, nodes[:, 1] + 2, nodes[:, 2] + 2]
    codes = all_codes("elastic", 3, 9)
    at = ctx.transfer_bytes()[0]
    got = ctx.gather(nl, codes[:16])
    assert ctx.transfer_bytes()[0] - at == 16 * n * 8
    same_bits(got, np.stack([quantity("elastic", 3, 9, c, rows) for c in codes[:16]]), f"gather n={n}")
    same_bits(ctx.gather(nl, codes[16:]), np.stack([quantity("elastic", 3, 9, c, rows) for c in codes[16:]]),
              f"gather n={n}, rest")
    nl.close()


def test_gather_refusals(G, gather_ctx):
    ctx, _ = gather_ctx
    for bad in ([[6, 0, 0]], [[0, 9, 0]], [[0, 0, 37]], [[0, -1, 0]], [[1, 1, 1], [0, 0, -1]]):
        with pytest.raises(G.GcmxError) as e:
            ctx.node_list(np.array(bad))
        assert e.value.status == ERR_INVALID_ARG, bad
    nl = ctx.node_list(np.array([[1, 2, 3]]))
    for codes in ([], [13], [64 + 9], [2] * 17):
        with pytest.raises(G.GcmxError) as e:
            ctx.gather(nl, codes)
        assert e.value.status == ERR_INVALID_ARG, codes
    other = random_context(G, [6, 9, 37], seed=1)
    with pytest.raises(G.GcmxError) as e:
        other.gather(nl, [2])  # a list belongs to the context it was created on
    assert e.value.status == ERR_INVALID_ARG
    other.close()


# -------------------------------------------------------------------- scan --

@pytest.mark.parametrize("sizes", [[6, 9, 37], [3, 4, 515]])
def test_scan(G, sizes):
    b = oracle_body(3, 2, sizes)
    random_state(b, 11, ghosts=True)
    ctx = G.Context(3, 2, sizes)
    ctx.upload(b.pde)
    inner = b.inner_view().reshape(-1, 9)
    at = ctx.transfer_bytes()[0]
    bad, mx = ctx.scan()
    assert ctx.transfer_bytes()[0] - at == 80
    assert bad == 0
    same_bits(mx, np.abs(inner).max(axis=0), f"max_abs {sizes}")
    # non-finite values in inner nodes are counted and left out of the maxima; one in a ghost is not seen
    iv = b.inner_view()
    iv[1, 2, 5, 3] = np.nan
    iv[sizes[0] - 1, sizes[1] - 1, sizes[2] - 1, 0] = np.inf
    iv[0, 0, 0, 8] = -np.inf
    iv[2, 3, sizes[2] - 2, 8] = np.nan
    b.pde.reshape(ctx.shape_all + (9,))[0, 0, 0, 4] = np.nan  # a ghost corner
    b.pde.reshape(ctx.shape_all + (9,))[3, 3, 1, 4] = np.inf  # a z ghost next to an inner node
    finite = np.where(np.isfinite(b.inner_view()), np.abs(b.inner_view()), 0.0).reshape(-1, 9).max(axis=0)
    ctx.upload(b.pde)
    bad, mx = ctx.scan()
    assert bad == 4
    same_bits(mx, finite, f"max_abs with plants {sizes}")
    # a component without a finite value reports 0.0
    b.inner_view()[..., 6] = np.nan
    ctx.upload(b.pde)
    bad, mx = ctx.scan()
    assert bad == 4 + int(np.prod(sizes)) and mx[6] == 0.0 and not np.signbit(mx[6])
    ctx.close()


# -------------------------------------------------- observation is read-only --

def test_observation_changes_no_state(G):
    sizes = [6, 9, 37]
    b = oracle_body(3, 2, sizes)
    random_state(b, 5, ghosts=False)
    seen, twin = context_for(b), context_for(b)
    tau = 0.9 / b.maximal_eigenvalue
    path = seen.effective_path
    assert path == twin.effective_path == "fused"
    nl = seen.node_list(np.array([[0, 0, 0], [5, 8, 36]]))
    for _ in range(2):
        seen.gather(nl, [PRESSURE, 2])
        seen.snapshot_box([0, 0, 0], sizes, [PRESSURE])
        seen.scan()
        assert seen.effective_path == path
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


def check_engine_files(H, make_task, bodies, D, detector_comp, detector_nodes, steps, steps_per_snap, tmp_path,
                       monkeypatch, chunk=None):
    """Run the task with VTK + SLICESNAP, then a twin engine step by step whose
    layers (pdeAll) go through the GPU-free writer: the .vts files must be equal
    byte for byte, the text files equal to the same series formed here from the
    twin's layers.  Returns the observed engine."""
    monkeypatch.chdir(tmp_path)
    t = make_task()
    t.add_snapshotter("VTK")
    t.add_snapshotter("SLICESNAP")
    t.output_directory = "seen"
    if chunk:
        t.set_vtk_chunk_bytes(chunk)
    he = H.Engine(t)
    he.run()
    assert he.steps == steps
    twin = H.Engine(make_task())
    times, seismo = [], []
    for step in range(steps + 1):
        if step:
            twin.run_steps(1)
        if step % steps_per_snap:
            continue
        for i in bodies:
            pde = twin.pde(i)
            stem = f"snapshots/seen/%s/mesh{i}core00snap{step:04d}"
            H.write_vtk(t, i, f"want/{i}_{step}.vts", pde)
            assert read(stem % "vtk" + ".vts") == read(f"want/{i}_{step}.vts"), (i, step)
            bs = 2
            inn = pde[tuple(slice(bs, -bs) for _ in range(D))]
            centre = tuple(s // 2 for s in inn.shape[:D - 1])
            col = inn[centre][:, D - 1]
            want = "".join(f"{float(z):g}\t{float(v):g}\t\n" for z, v in zip(range(len(col)), col))
            assert read(stem % "zaxis" + ".txt").decode() == want, (i, step)
            if i != 0:
                continue
            acc = 0.0
            vals = [float(inn[n][detector_comp]) for n in detector_nodes(inn.shape[:D])]
            for v in vals:
                acc += v
            times.append(twin.time)
            seismo.append(float(np.float32(acc / len(vals))))
            want = "".join(f"{a:g}\t{c:g}\t\n" for a, c in zip(times, seismo))
            assert read(stem % "detector" + ".txt").decode() == want, (i, step)
    return he


def cube_task():
    N = 12
    s = spec(3, 2, [1, 1, 1], {0: ([N] * 3, [0] * 3)}, 0.9, (4, 2, 1), snaps=3, steps_per_snap=2,
             quantities=[(("sphere", 3.0, (6.0, 6.0, 6.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_vtk_quantities(["PRESSURE"])
    t.set_detector(["Szz"], ("box", (-1, -1, -1), (7.5, 100, 100)), 0)
    return t


@pytest.mark.parametrize("chunk", [None, 1024])
def test_engine_snapshotters_move_no_layer(H, tmp_path, monkeypatch, chunk):
    """The task of test_engine_snapshotters (12^3, VTK + SLICESNAP): the same files,
    and the whole run copies less than one layer to the host (eight before)."""
    nodes = lambda shape: [(x, y, shape[2] - 1) for x in range(shape[0]) for y in range(shape[1]) if x < 7.5]
    he = check_engine_files(H, cube_task, [0], 3, 8, nodes, 6, 2, tmp_path, monkeypatch, chunk)
    layer = 16 ** 3 * 9 * 8
    d2h, h2d = he.transfer_bytes(0)
    assert 0 < d2h < layer, (d2h, layer)
    # four snapshots of Velocity + pressure, a column and the detector face
    assert d2h == 4 * (12 ** 3 * 16 + 12 * 8 + 8 * 12 * 8)
    assert h2d >= layer  # the set-up upload is counted too


def stack_task():
    X, Y, Z = 10, 12, 64
    cubics = {0: ([X, 5, Z], [0, 0, 0]), 1: ([X, 7, Z], [0, 5, 0])}
    s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=2, steps_per_snap=2,
             quantities=[(("sphere", 5.0, (X / 2, 3.5, Z / 2)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_vtk_quantities(["PRESSURE", "Vy"])
    t.set_detector(["Syy"], ("box", (-1, -1, -1), (100, 100, 100)), 0)
    return t


def test_engine_stack_members_snapshot_their_own_nodes(H, tmp_path, monkeypatch):
    """Two bodies stacked along y (5 + 7 of [10, 12, 64]) run as one grid: each
    member's files hold its own nodes, read from the stack's context at its offset."""
    nodes = lambda shape: [(x, y, shape[2] - 1) for x in range(shape[0]) for y in range(shape[1])]
    he = check_engine_files(H, stack_task, [0, 1], 3, 6, nodes, 4, 2, tmp_path, monkeypatch)
    assert he.last_path(0) == "fused" and he.last_path(1) == "fused"
    d2h = he.transfer_bytes(0)[0]
    assert d2h == he.transfer_bytes(1)[0]  # one context behind both members
    smallest_member_layer = 14 * 9 * 68 * 9 * 8
    assert 0 < d2h < smallest_member_layer, (d2h, smallest_member_layer)


def acoustic_task(H):
    t = H.Task()
    t.dimensionality = 2
    t.border_size = 2
    t.h = [1.0, 1.0]
    t.courant = 1.0
    t.number_of_snaps = 4
    t.steps_per_snap = 2
    t.add_body(0, [40, 30], [0, 0], model="acoustic")
    t.set_default_material(1.0, 1.0, 0.0)
    t.add_initial_quantity(("sphere", 6.0, (20.0, 15.0, 0.0)), "PRESSURE", 10.0)
    # the launcher's face condition (launcher/main.cpp:422-467): PRESSURE = 0 on y-
    t.add_border_condition(0, 1, ("box", (-1e3, -1e3, -1e3), (1e3, 1e-5, 1e3)), {"PRESSURE": lambda time: 0.0})
    t.set_vtk_quantities(["PRESSURE", "Vx"])
    t.set_detector(["PRESSURE"], ("box", (9.5, -1, -1), (30.5, 100, 100)), 0)
    return t


def test_engine_acoustic_2d(H, tmp_path, monkeypatch):
    nodes = lambda shape: [(x, shape[1] - 1) for x in range(shape[0]) if 9.5 < x < 30.5]
    he = check_engine_files(H, lambda: acoustic_task(H), [0], 2, 2, nodes, 8, 2, tmp_path, monkeypatch)
    assert he.matrix_structure(0) == 3
    # A layer here is 24 bytes per node, barely more than one snapshot's 20, so the
    # run is held to exactly its outputs: five snapshots of Velocity + two quantities,
    # the column and the 21 detector nodes.
    assert he.transfer_bytes(0)[0] == 5 * (40 * 30 * 20 + 30 * 8 + 21 * 8)
