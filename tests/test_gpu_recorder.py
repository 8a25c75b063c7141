"""Recorders (gcmx_recorder_*, k_record): samples of quantities at receivers kept
on the device and read in batches, and the engine's snapshotters on top of them.

Node recorders are held to gcmx_gather at the same moment, bit for bit; point
recorders to tests/recorder_ref.py (the rule of include/gcmx.h restated in
numpy) applied to the downloaded layer; the buffered SliceSnapshotter to the
unbuffered one's files; the DETECTOR snapshotter to a twin engine's layers
pushed through recorder_ref.py."""
import os

import numpy as np
import pytest

from tests import acoustic_ref as A
from tests import recorder_ref as R
from tests.taskspec import host_task, spec

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 5
PRESSURE = 12
BS = 2


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


# ---------------------------------------------------------------- contexts --

def make_context(G, sizes, model="elastic", seed=None, scale=1.0):
    """(context, tau): materials set, the whole layer random (ghosts included),
    Courant 0.9 on a unit grid."""
    D = len(sizes)
    if model == "acoustic":
        U, U1, L = A.acoustic_tables(D, 2.0, 8.0)  # c = 2
        tau = 0.9 / 2.0
    else:
        from gcm_amd.host import isotropic_elastic_matrices
        U, U1, L = isotropic_elastic_matrices(D, 4.0, 2.0, 1.0)  # c1 = 1
        tau = 0.9
    ctx = G.Context(D, BS, sizes, model=model)
    ctx.set_materials(U[None], U1[None], L[None])
    rng = np.random.default_rng(sum(sizes) + D if seed is None else seed)
    ctx.upload(rng.uniform(-1, 1, (ctx.n_all, ctx.M)) * scale)
    return ctx, tau


CASES = {"iso3": ([4, 5, 64], "elastic"), "el2": ([21, 70], "elastic"), "el1": ([50], "elastic"),
         "ac3": ([6, 9, 37], "acoustic")}


def all_codes(model, D, M):
    """Every component by GCMX_Q_COMPONENT, every named quantity the vector has, PRESSURE."""
    named = [2 + d for d in range(D)]
    if model == "elastic":
        named += [c for c, (i, j) in {5: (0, 0), 6: (0, 1), 7: (0, 2), 8: (1, 1), 9: (1, 2),
                                      10: (2, 2)}.items() if i < D and j < D]
    return [PRESSURE] + [64 + c for c in range(M)] + named


def sixteen(codes):
    return [codes[i % len(codes)] for i in range(16)]


def random_nodes(sizes, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, s, n) for s in sizes], axis=1).astype(np.int32)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} differ; first at "
                           f"{tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r} "
                           f"want {want[tuple(np.argwhere(bad)[0])]!r}")


def layer_of(ctx):
    return ctx.download().reshape(ctx.shape_all + (ctx.M,))


def script(D):
    """Both layer parities: a step, three stages (the layers swap after each), a step."""
    return [("step", None), ("stage", 0), ("stage", 1 % D), ("stage", 2 % D), ("step", None)]


def advance(ctx, op, axis, tau):
    if op == "step":
        ctx.step(tau)
    else:
        ctx.stage(axis, tau)


def check_against_gather(ctx, tau, nodes, qsets, what):
    """After every call of the script: record, read that sample, gather -- equal
    bit for bit; at the end the whole record equals the gathers in order."""
    nl = ctx.node_list(nodes)
    recs = [ctx.recorder(nl, q, 8) for q in qsets]
    want = [[] for _ in qsets]
    for op, axis in script(ctx.dim):
        advance(ctx, op, axis, tau)
        for r, q, w in zip(recs, qsets, want):
            ctx.record(r)
            w.append(ctx.gather(nl, q))
            same_bits(r.read(r.count - 1, 1)[0], w[-1], f"{what} {q} after {op} {axis}")
    for r, q, w in zip(recs, qsets, want):
        assert r.count == len(w)
        got = r.read()
        assert got.shape == (len(w), len(q), len(nodes))
        same_bits(got, np.stack(w), f"{what} {q} whole record")
        assert len({g.tobytes() for g in got}) > 1, "the samples must differ from call to call"
        r.close()


# ------------------------------------------------- node recorders == gather --

@pytest.mark.parametrize("case", list(CASES))
def test_one_receiver_one_quantity(G, case):
    """n = 1, n_q = 1: a component, PRESSURE, GCMX_Q_COMPONENT."""
    sizes, model = CASES[case]
    ctx, tau = make_context(G, sizes, model)
    node = np.array([[s // 2 for s in sizes]], np.int32)
    check_against_gather(ctx, tau, node, [[2], [PRESSURE], [G.gcmx.Q_COMPONENT(ctx.M - 1)]], case)
    ctx.close()


@pytest.mark.parametrize("case", list(CASES))
def test_two_blocks_and_a_tail(G, case):
    """n = 37, n_q = 16: 592 threads, two full blocks and a tail."""
    sizes, model = CASES[case]
    ctx, tau = make_context(G, sizes, model)
    codes = sixteen(all_codes(model, ctx.dim, ctx.M))
    assert PRESSURE in codes and 2 in codes and 64 in codes
    check_against_gather(ctx, tau, random_nodes(sizes, 37, 37), [codes], case)
    ctx.close()


@pytest.mark.parametrize("pads", [{"GCMX_ROW_PAD": "1"}, {"GCMX_PLANE_PAD": "3"},
                                  {"GCMX_ROW_PAD": "1", "GCMX_PLANE_PAD": "1"}])
def test_padded_layouts(G, monkeypatch, pads):
    for k, v in pads.items():
        monkeypatch.setenv(k, v)
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes)
    codes = sixteen(all_codes("elastic", 3, 9))
    check_against_gather(ctx, tau, random_nodes(sizes, 37, 5), [codes], f"padded {pads}")
    rng = np.random.default_rng(9)
    pos = rng.uniform(0, 1, (11, 3)) * (np.array(sizes) - 1)
    rec = ctx.point_recorder(pos, codes, 1)
    ctx.record(rec)
    want = R.sample(layer_of(ctx), BS, "elastic", pos, codes)
    same_bits(rec.read()[0] + 0.0, want + 0.0, f"points, padded {pads}")
    ctx.close()


def test_subnormal_state(G):
    """A state scaled by 2^-1060: every value a subnormal, kept bit for bit."""
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes, scale=2.0 ** -1060)
    layer = ctx.download()
    assert np.all(np.abs(layer) < np.finfo(np.float64).tiny) and np.count_nonzero(layer) > layer.size // 2
    codes = sixteen(all_codes("elastic", 3, 9))
    nodes = random_nodes(sizes, 37, 11)
    nl = ctx.node_list(nodes)
    rec = ctx.recorder(nl, codes, 2)
    ctx.record(rec)
    first = ctx.gather(nl, codes)
    assert np.count_nonzero(first) > first.size // 2
    ctx.step(tau)
    ctx.record(rec)
    same_bits(rec.read(), np.stack([first, ctx.gather(nl, codes)]), "subnormals")
    ctx.close()


# ------------------------------------------------------------- bookkeeping --

@pytest.mark.parametrize("capacity", [1, 3])
def test_capacity_reads_and_resets(G, capacity):
    """7 samples through a recorder of capacity 1 or 3: read and reset when full."""
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes)
    nodes = random_nodes(sizes, 5, 3)
    nl = ctx.node_list(nodes)
    q = [4, PRESSURE]
    rec = ctx.recorder(nl, q, capacity)
    nl.close()  # the recorder copied the list
    nl = ctx.node_list(nodes)
    want, got = [], []
    assert rec.count == 0
    for i in range(7):
        if rec.count == capacity:
            got.extend(rec.read())
            rec.reset()
            assert rec.count == 0
        ctx.step(tau)
        ctx.record(rec)
        want.append(ctx.gather(nl, q))
        assert rec.count == len(want) - len(got)
    got.extend(rec.read())
    same_bits(np.stack(got), np.stack(want), f"capacity {capacity}")
    ctx.close()


def test_full_recorder_and_ranges(G):
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes)
    nl = ctx.node_list(random_nodes(sizes, 5, 4))
    q = [2, 64 + 8]
    rec = ctx.recorder(nl, q, 3)
    with pytest.raises(G.GcmxError) as e:  # nothing held yet
        rec.read(0, 1)
    assert e.value.status == ERR_INVALID_ARG
    for _ in range(3):
        ctx.step(tau)
        ctx.record(rec)
    held = rec.read()
    ctx.step(tau)  # the layer moves on: a sample written now would differ
    with pytest.raises(G.GcmxError) as e:
        ctx.record(rec)
    assert e.value.status == ERR_STATE
    assert rec.count == 3
    same_bits(rec.read(), held, "a refused record changes nothing")
    same_bits(rec.read(1, 2), held[1:], "first = 1, count = 2")
    same_bits(rec.read(2), held[2:], "first = 2")
    for first, count in [(-1, 1), (0, 0), (0, -1), (0, 4), (3, 1), (2, 2), (2 ** 31 - 1, 1)]:
        with pytest.raises(G.GcmxError) as e:
            rec.read(first, count)
        assert e.value.status == ERR_INVALID_ARG, (first, count)
    # creation refusals
    for bad in (lambda: ctx.recorder(nl, q, 0), lambda: ctx.recorder(nl, [], 1), lambda: ctx.recorder(nl, [2] * 17, 1),
                lambda: ctx.recorder(nl, [11], 1), lambda: ctx.point_recorder([[0.0, 0.0, 64.0]], q, 1),
                lambda: ctx.point_recorder([[0.0, float("nan"), 1.0]], q, 1),
                lambda: ctx.point_recorder([[-0.25, 0.0, 1.0]], q, 1), lambda: ctx.point_recorder([[1.0, 1.0, 1.0]], q, 0)):
        with pytest.raises(G.GcmxError) as e:
            bad()
        assert e.value.status == ERR_INVALID_ARG
    flat = G.Context(3, 1, [1, 5, 64])  # sizes_d = 1: no pair of nodes along x
    with pytest.raises(G.GcmxError) as e:
        flat.point_recorder([[0.0, 1.0, 1.0]], [2], 1)
    assert e.value.status == ERR_INVALID_ARG
    flat.close()
    ctx.close()


def test_other_context_and_detach(G):
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes)
    other, _ = make_context(G, sizes, seed=77)
    nl = ctx.node_list(random_nodes(sizes, 5, 6))
    q = [3, PRESSURE]
    rec = ctx.recorder(nl, q, 4)
    with pytest.raises(G.GcmxError) as e:  # a list of another context
        other.recorder(nl, q, 4)
    assert e.value.status == ERR_INVALID_ARG
    for _ in range(2):
        ctx.step(tau)
        ctx.record(rec)
    with pytest.raises(G.GcmxError) as e:  # a recorder of another context
        other.record(rec)
    assert e.value.status == ERR_INVALID_ARG
    assert rec.count == 2
    held = rec.read()
    ctx.step(tau)
    ctx.record(rec)  # still in flight when the context goes: gcmx_destroy waits for it
    last = ctx.gather(nl, q)
    ctx.close()
    assert rec.count == 3
    same_bits(rec.read(), np.concatenate([held, last[None]]), "read after gcmx_destroy")
    same_bits(rec.read(2, 1)[0], last, "read after gcmx_destroy, one sample")
    with pytest.raises(G.GcmxError) as e:  # detached
        other.record(rec)
    assert e.value.status == ERR_INVALID_ARG
    assert rec.count == 3
    rec.close()
    other.close()


def test_transfer_bytes(G):
    sizes = [4, 5, 64]
    ctx, tau = make_context(G, sizes)
    n, q = 37, [2, 3, PRESSURE]
    rec = ctx.recorder(ctx.node_list(random_nodes(sizes, n, 8)), q, 5)
    pts = ctx.point_recorder(np.full((n, 3), 1.5), q, 5)
    before = ctx.transfer_bytes()
    for _ in range(5):
        ctx.step(tau)
        ctx.record(rec)
        ctx.record(pts)
    assert ctx.transfer_bytes() == before, "record copies nothing"
    rec.read()
    assert ctx.transfer_bytes() == (before[0] + 5 * len(q) * n * 8, before[1])
    rec.read(1, 2)
    pts.read(4, 1)
    assert ctx.transfer_bytes() == (before[0] + (5 + 2 + 1) * len(q) * n * 8, before[1])
    rec.reset()
    assert ctx.transfer_bytes() == (before[0] + 8 * len(q) * n * 8, before[1])
    ctx.close()


def test_profile_bucket(G):
    ctx, tau = make_context(G, [4, 5, 64])
    rec = ctx.recorder(ctx.node_list(random_nodes(ctx.sizes, 3, 1)), [2], 2)
    ctx.profile(True)
    ctx.record(rec)
    ctx.record(rec)
    assert ctx.profile_read()["record_q"]["launches"] == 2
    ctx.close()


# ---------------------------------------------------------- point recorders --

POINT_CASES = {"el1": ([50], "elastic", True), "el2": ([21, 70], "elastic", True), "iso3": ([4, 5, 64], "elastic", True),
               "ac1": ([50], "acoustic", True), "ac2": ([21, 70], "acoustic", True), "ac3": ([6, 9, 37], "acoustic", True),
               "two2": ([2, 9], "elastic", False), "two3": ([5, 2, 64], "elastic", False),
               "two3ac": ([2, 2, 2], "acoustic", False)}


@pytest.mark.parametrize("case", list(POINT_CASES))
def test_points_against_the_restated_rule(G, case):
    """Random positions, positions on nodes (the node's value), the upper edge,
    sizes_d = 2; every quantity of the vector, the elastic PRESSURE included."""
    sizes, model, stepped = POINT_CASES[case]
    D = len(sizes)
    ctx, tau = make_context(G, sizes, model)
    codes = all_codes(model, D, ctx.M)
    top = np.array(sizes, np.float64) - 1
    rng = np.random.default_rng(len(case) + sum(sizes))
    nodes = random_nodes(sizes, 9, 21)
    edge = rng.uniform(0, 1, (6, D)) * top
    for i in range(6):
        edge[i, i % D] = top[i % D]  # on the upper face of one axis
    pos = np.concatenate([rng.uniform(0, 1, (20, D)) * top, nodes.astype(np.float64), edge, top[None], np.zeros((1, D))])
    parts = [codes[:16], codes[16:]] if len(codes) > 16 else [codes]  # GCMX_MAX_BORDER_Q per recorder
    recs = [ctx.point_recorder(pos, part, 2) for part in parts]
    nl = ctx.node_list(nodes)
    for sample in range(2 if stepped else 1):
        if sample:
            ctx.step(tau)
        layer = layer_of(ctx)
        for rec, part in zip(recs, parts):
            ctx.record(rec)
            got = rec.read(sample, 1)[0]
            want = R.sample(layer, BS, model, pos, part)
            same_bits(got + 0.0, want + 0.0, f"{case} sample {sample}")
            # a point on a node is the node
            same_bits(got[:, 20:29] + 0.0, ctx.gather(nl, part) + 0.0, f"{case} on nodes")
    ctx.close()


# ------------------------------------------------------------- slab groups --

def test_slab_group(G):
    """Two X slabs of [16, 6, 64] as an in-process group: each slab's recorder
    equals its gather over three steps (record waits for no exchange), and the
    group stays bitwise the undivided grid."""
    from gcm_amd.host import isotropic_elastic_matrices
    U, U1, L = isotropic_elastic_matrices(3, 4.0, 2.0, 1.0)
    X, Y, Z, seed = 8, 6, 64, 0x5EED

    def make(sizes, x0):
        c = G.Context(3, BS, sizes, start=[x0, 0, 0])
        c.set_materials(U[None], U1[None], L[None])
        c.fill_random([2 * X, Y, Z], seed)
        return c
    slabs = [make([X, Y, Z], 0), make([X, Y, Z], X)]
    G.gcmx.comm_init_local(slabs)
    whole = make([2 * X, Y, Z], 0)
    q = [2, PRESSURE, 64 + 8]
    nodes = [random_nodes([X, Y, Z], 37, 50 + i) for i in range(2)]
    for i in range(2):  # the planes next to the seam and the outer ones
        nodes[i][:4, 0] = [0, 1, X - 2, X - 1]
    lists = [c.node_list(n) for c, n in zip(slabs, nodes)]
    recs = [c.recorder(nl, q, 3) for c, nl in zip(slabs, lists)]
    want = [[], []]
    for _ in range(3):
        G.gcmx.local_group_steps(slabs, 0.9, 1)
        whole.step(0.9)
        for c, r in zip(slabs, recs):
            c.record(r)  # before any call that waits for the exchange
        for c, nl, w in zip(slabs, lists, want):
            w.append(c.gather(nl, q))
    for r, w in zip(recs, want):
        same_bits(r.read(), np.stack(w), "slab recorder")
    inner = lambda c: layer_of(c)[BS:-BS, BS:-BS, BS:-BS]
    got = np.concatenate([inner(c) for c in slabs], axis=0)
    assert np.array_equal(got.view(np.uint64), inner(whole).view(np.uint64))
    for c in slabs + [whole]:
        c.close()


# ------------------------------------------------------------------ engine --

def read(path):
    with open(path, "rb") as f:
        return f.read()


def tree(root):
    out = {}
    for folder in ("zaxis", "detector"):
        d = os.path.join(root, folder)
        for name in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            out[folder + "/" + name] = read(os.path.join(d, name))
    return out


def cube_task():
    """The 12^3 task of test_gpu_observe.py's snapshotter tests, a snapshot every step: 7 of them."""
    s = spec(3, 2, [1, 1, 1], {0: ([12] * 3, [0] * 3)}, 0.9, (4, 2, 1), snaps=6, steps_per_snap=1,
             quantities=[(("sphere", 3.0, (6.0, 6.0, 6.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_detector(["Szz"], ("box", (-1, -1, -1), (7.5, 100, 100)), 0)
    return t


def stack_task():
    cubics = {0: ([10, 5, 64], [0, 0, 0]), 1: ([10, 7, 64], [0, 5, 0])}
    s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=6, steps_per_snap=1,
             quantities=[(("sphere", 5.0, (5.0, 3.5, 32.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_detector(["Syy"], ("box", (-1, -1, -1), (100, 100, 100)), 0)
    return t


@pytest.mark.parametrize("make_task,bodies", [(cube_task, [0]), (stack_task, [0, 1])], ids=["cube", "ystack"])
def test_engine_buffered_slice_snapshotter(H, tmp_path, monkeypatch, make_task, bodies):
    """bufferSteps 3 over 7 snapshots (a flush mid-run twice, one sample left for the
    final flush): the zaxis and detector trees of the unbuffered run byte for
    byte, and the same bytes device -> host."""
    monkeypatch.chdir(tmp_path)
    seen = {}
    for name, n in (("plain", 0), ("buffered", 3)):
        t = make_task()
        t.add_snapshotter("SLICESNAP")
        t.output_directory = name
        t.set_detector_buffer(n)
        he = H.Engine(t)
        he.run()
        assert he.steps == 6
        seen[name] = (tree(os.path.join("snapshots", name)), [he.transfer_bytes(i)[0] for i in bodies])
        del he
    plain, buffered = seen["plain"], seen["buffered"]
    want = {f"zaxis/mesh{i}core00snap{s:04d}.txt" for i in bodies for s in range(7)}
    want |= {f"detector/mesh0core00snap{s:04d}.txt" for s in range(7)}
    assert set(plain[0]) == want
    assert set(buffered[0]) == want
    for name in sorted(want):
        assert buffered[0][name] == plain[0][name], name
    assert len(plain[0]["detector/mesh0core00snap0006.txt"].splitlines()) == 7
    assert buffered[1] == plain[1] and plain[1][0] > 0


def receivers_2d_task(H):
    s = spec(2, 2, [0.5, 0.25], {0: ([21, 30], [3, -2])}, 0.9, (4, 2, 1), snaps=4, steps_per_snap=1,
             quantities=[(("sphere", 2.0, (6.5, 3.0, 0.0)), "PRESSURE", 10.0)])
    return host_task(s)


def receivers_3d_task(H):
    s = spec(3, 2, [1, 1, 1], {0: ([12] * 3, [0] * 3)}, 0.9, (4, 2, 1), snaps=4, steps_per_snap=1,
             quantities=[(("sphere", 3.0, (6.0, 6.0, 6.0)), "PRESSURE", 10.0)])
    return host_task(s)


RECEIVER_CASES = {
    "3d": (receivers_3d_task, [1.0, 1.0, 1.0], [0, 0, 0],
           [[3.3, 4.7, 5.2], [0.0, 0.0, 0.0], [11.0, 11.0, 11.0], [6.0, 6.0, 6.0], [2.5, 11.0, 0.25]],
           ["Vz", "PRESSURE", "Sxy"], [13.0, 3.0, 3.0]),
    "2d": (receivers_2d_task, [0.5, 0.25], [3, -2],
           [[1.5, -0.5], [11.5, 6.75], [6.6, 3.1], [4.0, 0.0], [7.123, 6.75]],
           ["Vx", "Sxy", "PRESSURE"], [1.25, 0.0]),
}


@pytest.mark.parametrize("case", list(RECEIVER_CASES))
def test_engine_detector_snapshotter(G, H, tmp_path, monkeypatch, case):
    """bufferSteps 2 over 5 snapshots: three files (2 + 2 + 1 rows) which together
    are the record of a twin engine's layers pushed through recorder_ref.py."""
    make_task, h, start, points, names, outside = RECEIVER_CASES[case]
    D = len(h)
    monkeypatch.chdir(tmp_path)
    t = make_task(H)
    t.add_snapshotter("DETECTOR")
    t.output_directory = "seen"
    t.set_receivers(points, names, 0, 2)
    he = H.Engine(t)
    he.run()
    assert he.steps == 4
    folder = os.path.join("snapshots", "seen", "receivers")
    assert sorted(os.listdir(folder)) == [f"mesh0core00snap{s:04d}.txt" for s in (0, 2, 4)]
    rows = []
    for s, n in ((0, 2), (2, 2), (4, 1)):
        text = read(os.path.join(folder, f"mesh0core00snap{s:04d}.txt")).decode()
        lines = text.split("\n")
        assert lines[-1] == "" and len(lines) == n + 1, (s, lines)
        for line in lines[:-1]:
            fields = line.split("\t")
            assert len(fields) == 1 + len(names) * len(points)
            assert all(f == "%.17g" % float(f) for f in fields)
            rows.append([float(f) for f in fields])
    codes = [G.gcmx.QUANTITY_CODES[n] for n in names]
    # pos_d = (p_d - coords(0)_d) / h_d with coords(0)_d = start_d h_d + 0 h_d, as the host forms it
    pos = [[(p[d] - (float(start[d]) * h[d] + 0.0 * h[d])) / h[d] for d in range(D)] for p in points]
    twin = H.Engine(make_task(H))
    for step in range(5):
        if step:
            twin.run_steps(1)
        want = R.sample(np.asarray(twin.pde(0)), BS, "elastic", pos, codes)
        assert rows[step][0] == twin.time, step
        assert rows[step][1:] == want.reshape(-1).tolist(), step
    assert any(v != 0.0 for v in rows[4][1:])
    # a point outside the body's inner nodes
    t = make_task(H)
    t.add_snapshotter("DETECTOR")
    t.output_directory = "refused"
    t.set_receivers(points + [outside], names, 0, 2)
    with pytest.raises(H.GcmException):
        H.Engine(t).run()
    # another body's receivers: nothing is written
    t = make_task(H)
    t.add_snapshotter("DETECTOR")
    t.output_directory = "other"
    t.set_receivers(points, names, 5, 2)
    H.Engine(t).run()
    assert not os.path.exists(os.path.join("snapshots", "other", "receivers"))
