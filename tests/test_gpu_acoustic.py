"""Acoustic contexts (gcmx_create_model, M = D + 1): the generic stages in 1-,
2- and 3-D, the one-pass 3-D step k_step_acoustic and its dispatch, border
conditions and refusals, bitwise against the oracle's stage sequence run with
the acoustic tables of tests/acoustic_ref.py (a numpy restatement of the
reference's AcousticModel, never the product's).  Unless stated otherwise a case
takes a random state on the inner nodes with zero ghosts and runs 3 steps."""
import math

import numpy as np
import pytest

from tests import acoustic_ref as A
from tests.helpers import assert_same, assert_same_inner, random_materials, random_state

pytestmark = pytest.mark.gpu

H_A = (0.5, 0.4, 0.3)
RHO, LAM = 2.0, 8.0  # c = 2
C = 2.0
ERR_INVALID_ARG, ERR_CFL, ERR_UNSUPPORTED = 1, 2, 6
Q = {"Vx": 2, "Vy": 3, "Vz": 4, "Sxx": 5, "PRESSURE": 12}


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def courant_tau(b, courant=0.9):
    return courant * min(b.h[:b.D]) / b.maximal_eigenvalue


def kernel_names(ctx):
    return [v["kernel"] for v in ctx.profile_read().values() if v["launches"] > 0]


def zt_of(Z):
    return next(t for t in (64, 128, 256, 512, 1024) if Z <= t)


def run_case(bs, sizes, h=H_A, tau=None, steps=3, setup=None, seed=None, path=None, want_path="fused"):
    D = len(sizes)
    b = A.acoustic_body(D, bs, sizes, h=h[:D], rho=RHO, lam=LAM)
    random_state(b, seed=sum(sizes) + bs if seed is None else seed, ghosts=False)
    ctx = A.context_for(b, path=path)
    assert ctx.model == "acoustic" and ctx.M == D + 1
    if setup is not None:
        setup(ctx)
    tau = courant_tau(b) if tau is None else tau
    ctx.profile(True)
    for step in range(steps):
        A.step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == want_path, f"step {step} ran {ctx.last_path}"
        assert_same(ctx, b, f"acoustic bs {bs} {sizes} step {step}")
    names = kernel_names(ctx)
    ctx.close()
    return names


# ------------------------------------------------------------ recognition --

def test_recognition(G):
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    ctx = A.context_for(b)
    assert ctx.matrix_structure() == 3
    assert ctx.effective_path == "fused"
    ctx.close()

    U, U1, L = (a.copy() for a in A.acoustic_tables(3, RHO, LAM))
    assert U[1, 2, 3] == 0.0
    U[1, 2, 3] = 1e-3  # one structural zero: a zero mode that reads the pressure
    b2 = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, tables=(U, U1, L))
    ctx = A.context_for(b2)
    assert ctx.matrix_structure() == 0
    assert ctx.effective_path == "generic"
    random_state(b2, seed=3, ghosts=False)
    ctx.upload(b2.pde)
    tau = courant_tau(b2)
    A.step(b2, tau)
    ctx.step(tau)
    assert ctx.last_path == "generic"
    assert_same(ctx, b2, "general matrices on an acoustic context")
    ctx.close()

    from tests.helpers import context_for, oracle_body
    ctx = context_for(oracle_body(3, 2, [6, 9, 37]))
    assert ctx.matrix_structure() == 1 and ctx.model == "elastic" and ctx.M == 9
    ctx.close()


def test_zero_mode_signs_are_both_accepted(G):
    """The reference's tangents carry signs like (0, -1); flipping a zero mode's
    sign in U and U1 together keeps structure 3 and the bits."""
    U, U1, L = (a.copy() for a in A.acoustic_tables(3, RHO, LAM))
    assert (U[:, 2:, :3] < 0).any(), "the restatement has no negative tangent to begin with"
    for s in range(3):
        U[s, 2] = -U[s, 2]
        U1[s, :, 2] = -U1[s, :, 2]
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, tables=(U, U1, L))
    ref = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    random_state(b, seed=5, ghosts=False)
    ref.pde[:] = b.pde
    ctx = A.context_for(b)
    assert ctx.matrix_structure() == 3 and ctx.effective_path == "fused"
    tau = courant_tau(b)
    for _ in range(3):
        A.step(b, tau)
        A.step(ref, tau)
        ctx.step(tau)
    assert_same(ctx, b, "flipped zero modes")
    assert np.array_equal(b.pde, ref.pde)
    ctx.close()


# ---------------------------------------------------------- generic stages --

@pytest.mark.parametrize("sizes,bs,path", [([40], 2, None), ([15, 11], 2, None), ([9, 70], 1, None),
                                           ([5, 6, 70], 2, "generic")])
def test_generic_stages(G, sizes, bs, path):
    names = run_case(bs, sizes, path=G.PATH_GENERIC if path else None, want_path="generic")
    assert names == ["k_stage_generic"], names


@pytest.mark.parametrize("sizes,bs", [([40], 2), ([15, 11], 2), ([5, 6, 70], 2)])
def test_stages_equal_step(G, sizes, bs):
    D = len(sizes)
    b = A.acoustic_body(D, bs, sizes, h=H_A[:D], rho=RHO, lam=LAM)
    random_state(b, seed=21, ghosts=False)
    a, c = A.context_for(b), A.context_for(b)
    tau = courant_tau(b)
    for _ in range(3):
        A.step(b, tau)
        a.step(tau)
        for s in range(D):
            c.stage(s, tau)
    assert c.last_path == "generic"
    assert_same(a, b, "step")
    assert_same(c, b, "stages")
    a.close()
    c.close()


@pytest.mark.parametrize("sizes,bs", [([15, 11], 2), ([5, 6, 70], 2), ([40], 1)])
def test_per_node_materials_run_the_generic_stages(G, sizes, bs):
    """Two acoustic materials with random per-node ids: structure 0, the HETERO
    instances of k_stage_generic, bitwise against the oracle's per-node stage; and
    the transition: the same context is structure 3 / fused (3-D) before the ids
    are set and after they are cleared again."""
    D = len(sizes)
    b = A.acoustic_body(D, bs, sizes, h=H_A[:D], rho=RHO, lam=LAM)
    b.tables = [A.acoustic_tables(D, RHO, LAM), A.acoustic_tables(D, 3.0, 5.0)]
    b.maximal_eigenvalue = max(A.max_eigenvalue(t[2]) for t in b.tables)
    random_materials(b, seed=41)
    random_state(b, seed=42, ghosts=False)
    import gcm_amd
    ctx = gcm_amd.Context(D, bs, sizes, h=H_A[:D], model="acoustic")
    one = b.tables[0]
    ctx.set_materials(one[0][None], one[1][None], one[2][None])
    assert ctx.matrix_structure() == 3
    assert ctx.effective_path == ("fused" if D == 3 else "generic")
    U, U1, L = (np.stack([t[i] for t in b.tables]) for i in range(3))
    ctx.set_materials(U, U1, L)
    ctx.set_material_ids(b.mat_id)
    assert ctx.matrix_structure() == 0 and ctx.effective_path == "generic"
    ctx.upload(b.pde)
    tau = courant_tau(b)
    ctx.profile(True)
    for step in range(3):
        A.step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == "generic"
        assert_same(ctx, b, f"per-node materials {sizes} step {step}")
    assert kernel_names(ctx) == ["k_stage_generic"]
    ctx.set_material_ids(None)
    ctx.set_materials(one[0][None], one[1][None], one[2][None])
    assert ctx.matrix_structure() == 3
    assert ctx.effective_path == ("fused" if D == 3 else "generic")
    ctx.close()


# ------------------------------------------------------------------ shapes --

@pytest.mark.parametrize("sizes,bs", [([6, 9, 37], 2),    # ZT 64 with idle lanes
                                      ([4, 5, 64], 2),    # no idle lane
                                      ([4, 5, 65], 2),    # ZT 128
                                      ([4, 2, 4], 2),     # the minimum: Y = bs, Z = 2 bs
                                      ([3, 4, 515], 2),   # ZT 1024
                                      ([6, 9, 37], 1),
                                      ([5, 7, 20], 3)])
def test_shapes(G, sizes, bs):
    names = run_case(bs, sizes)
    assert names == [f"k_step_acoustic<{bs}, {zt_of(sizes[2])}, KF0>"], names


@pytest.mark.parametrize("rows", [4, 1])
def test_chunk_seams(G, rows):
    """Partial last chunk, a prologue at both edges of every chunk."""
    names = run_case(2, [6, 9, 37], setup=lambda c: c.set_schedule(G.SCHED_SINGLE, rows_per_block=rows))
    assert names == ["k_step_acoustic<2, 64, KF0>"], names


# ------------------------------------------------------------------- !KF0 --

@pytest.mark.parametrize("sizes,bs,tau", [([6, 9, 37], 2, 1.0 / C),   # q = 1 exactly: the foot on a node
                                          ([6, 9, 37], 2, 1.5 / C),
                                          ([5, 4, 6], 3, 2.2 / C)])
def test_foot_beyond_the_first_interval(G, sizes, bs, tau):
    h = (1.0, 1.0, 1.0)
    L = A.acoustic_tables(3, RHO, LAM)[2]
    kf = [math.floor(abs(L[s, 0] * (-tau)) / h[s]) for s in range(3)]
    assert min(kf) >= 1 and max(kf) < bs, kf
    names = run_case(bs, sizes, h=h, tau=tau)
    assert names == [f"k_step_acoustic<{bs}, 64, !KF0>"], names


def test_courant_too_large_is_refused(G):
    b = A.acoustic_body(3, 2, [6, 9, 37], h=(1.0, 1.0, 1.0), rho=RHO, lam=LAM)
    ctx = A.context_for(b)
    with pytest.raises(G.GcmxError) as e:
        ctx.step(3.2 / C)  # q = 3.2 >= borderSize + 1
    assert e.value.status == ERR_CFL
    ctx.close()


# -------------------------------------------------------------- dispatch --

def test_paths_agree(G):
    """AUTO, GENERIC, SPLIT and gcmx_stage x 3 give identical bits."""
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    random_state(b, seed=11, ghosts=False)
    tau = courant_tau(b)
    ctxs = {"auto": A.context_for(b), "generic": A.context_for(b, path=G.PATH_GENERIC),
            "split": A.context_for(b, path=G.PATH_SPLIT), "stages": A.context_for(b)}
    for _ in range(3):
        A.step(b, tau)
        for name, c in ctxs.items():
            if name == "stages":
                for s in range(3):
                    c.stage(s, tau)
            else:
                c.step(tau)
    assert ctxs["auto"].last_path == "fused"
    assert ctxs["generic"].last_path == "generic" and ctxs["split"].last_path == "generic"
    assert ctxs["stages"].last_path == "generic"
    for name, c in ctxs.items():
        assert_same(c, b, name)
        c.close()


def test_padded_layout(G, monkeypatch):
    for k, v in {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"}.items():
        monkeypatch.setenv(k, v)
    c = G.Context(3, 2, [4, 4, 4], model="acoustic")
    g = c.geometry()
    c.close()
    assert g["stride"][1] % 2 == 1 and g["cs"] % 2 == 1, g
    names = run_case(2, [6, 9, 37])
    assert names == ["k_step_acoustic<2, 64, KF0>"], names


def test_fp_mode_is_accepted_and_changes_nothing(G):
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    random_state(b, seed=13, ghosts=False)
    tau = courant_tau(b)
    start = b.pde.copy()
    A.step(b, tau)
    for mode in (G.FP_FMA, G.FP_EXACT):
        ctx = A.context_for(b)
        ctx.upload(start)
        ctx.fp_mode = mode
        assert ctx.fp_mode == mode
        ctx.step(tau)
        assert ctx.last_path == "fused"
        assert_same(ctx, b, f"fp mode {mode}")
        ctx.close()


# ----------------------------------------------------------------- borders --

def border_plan(D, sizes):
    """PRESSURE = 0.25 on y-, Vx = 0.05 on x+, a time-dependent PRESSURE on the
    last axis' + face (z+ in 3-D; in 2-D that is y+)."""
    last = D - 1
    return [(1, -1, [("PRESSURE", lambda t: 0.25)]),
            (0, 1, [("Vx", lambda t: 0.05)]),
            (last, 1, [("PRESSURE", lambda t: 0.1 + 0.5 * t)])]


@pytest.mark.parametrize("sizes", [[6, 9, 37], [15, 11]])
def test_step_faces(G, sizes):
    D = len(sizes)
    b = A.acoustic_body(D, 2, sizes, h=H_A[:D], rho=RHO, lam=LAM)
    random_state(b, seed=31, ghosts=False)
    ctx = A.context_for(b)
    tau = courant_tau(b)
    plan = border_plan(D, sizes)
    t = 0.0
    for step in range(3):
        faces = [None] * (2 * D)
        for axis, side, vals in plan:
            faces[2 * axis + (side > 0)] = [(Q[q], f(t)) for q, f in vals]
        for s in range(D):
            for axis, side, vals in plan:
                if axis == s:
                    A.apply_border(b, axis, side, A.face_nodes(b, axis, side), [(q, f(t)) for q, f in vals])
            b.stage(s, tau)
        ctx.step_faces(tau, faces)
        assert ctx.last_path == "generic"
        assert_same_inner(ctx, b, f"faces step {step}")
        t += tau
    assert ctx.effective_path == "generic"
    A.step(b, tau)  # a later plain step stays on the stages: the faces' ghosts were written
    ctx.step(tau)
    assert ctx.last_path == "generic"
    assert_same_inner(ctx, b, "plain step after face steps")
    ctx.close()


@pytest.mark.parametrize("sizes", [[6, 9, 37], [15, 11]])
def test_border_fill(G, sizes):
    """gcmx_border_fill (node lists) before each stage, ghosts included."""
    D = len(sizes)
    b = A.acoustic_body(D, 2, sizes, h=H_A[:D], rho=RHO, lam=LAM)
    random_state(b, seed=32, ghosts=False)
    ctx = A.context_for(b)
    tau = courant_tau(b)
    plan = border_plan(D, sizes)
    t = 0.0
    for step in range(3):
        for s in range(D):
            for axis, side, vals in plan:
                if axis != s:
                    continue
                nodes = A.face_nodes(b, axis, side)
                now = [(q, f(t)) for q, f in vals]
                A.apply_border(b, axis, side, nodes, now)
                ctx.border_fill(axis, side, nodes, [Q[q] for q, _ in now], [v for _, v in now])
            b.stage(s, tau)
            ctx.stage(s, tau)
        assert_same_inner(ctx, b, f"border fill step {step}")
        t += tau
    assert ctx.effective_path == "generic"
    ctx.close()


def test_stress_quantity_is_refused(G):
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    ctx = A.context_for(b)
    with pytest.raises(G.GcmxError) as e:
        ctx.step_faces(courant_tau(b), [[(Q["Sxx"], 0.0)]] + [None] * 5)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(G.GcmxError) as e:
        ctx.border_fill(0, -1, A.face_nodes(b, 0, -1), [Q["Sxx"]], [0.0])
    assert e.value.status == ERR_INVALID_ARG
    ctx.close()


def test_partial_pressure_face_map(G):
    """A PRESSURE condition on part of the y- face and a Vz one on part of z+
    through gcmx_face_map_create; the nodes no condition covers keep their ghosts."""
    sizes = [6, 9, 12]
    b = A.acoustic_body(3, 2, sizes, h=H_A, rho=RHO, lam=LAM)
    random_state(b, seed=33, ghosts=False)
    ctx = A.context_for(b)
    tau = courant_tau(b)
    area_y = ("box", (0.4, -1.0, 0.5), (2.1, 1.0, 2.8))
    area_z = ("sphere", 1.2, (1.0, 1.6, 3.3))
    ny, nz = A.face_nodes(b, 1, -1, area_y), A.face_nodes(b, 2, 1, area_z)
    assert 0 < len(ny) < sizes[0] * sizes[2] and 0 < len(nz) < sizes[0] * sizes[1]
    my = np.full((sizes[0], sizes[2]), 255, dtype=np.uint8)
    my[ny[:, 0], ny[:, 2]] = 0
    mz = np.full((sizes[0], sizes[1]), 255, dtype=np.uint8)
    mz[nz[:, 0], nz[:, 1]] = 1
    fmap = ctx.face_map([None, None, my, None, None, mz])
    t = 0.0
    for step in range(3):
        conds = [[("PRESSURE", 0.3 - t)], [("Vz", 0.07)]]
        for s in range(3):
            if s == 1:
                A.apply_border(b, 1, -1, ny, conds[0])
            if s == 2:
                A.apply_border(b, 2, 1, nz, conds[1])
            b.stage(s, tau)
        ctx.step_face_map(tau, fmap, [[(Q[q], v) for q, v in c] for c in conds])
        assert ctx.last_path == "generic"
        assert_same_inner(ctx, b, f"face map step {step}")
        t += tau
    ctx.close()


# ---------------------------------------------------------------- refusals --

def test_refusals(G):
    b = A.acoustic_body(3, 2, [6, 9, 37], h=H_A, rho=RHO, lam=LAM)
    ctx, other = A.context_for(b), A.context_for(b)
    tau = courant_tau(b)
    for call in (lambda: ctx.step_ode(tau, [1.0]), lambda: ctx.ode_maxwell(tau, [1.0]),
                 lambda: G.comm_init_local([ctx, other]), lambda: ctx.comm_init_loopback()):
        with pytest.raises(G.GcmxError) as e:
            call()
        assert e.value.status == ERR_UNSUPPORTED, str(e.value)
    ctx.step(tau)  # the context still steps
    assert ctx.last_path == "fused"
    ctx.close()
    other.close()


# ------------------------------------------------------------------ engine --

@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def host_task(H, D, bs, sizes, h, courant, material, snaps, quantities=(), borders=()):
    t = H.Task()
    t.dimensionality = D
    t.border_size = bs
    t.h = list(h)
    t.courant = courant
    t.number_of_snaps = snaps
    t.steps_per_snap = 1
    t.add_body(0, list(sizes), [0] * D, model="acoustic")
    t.set_default_material(*material)
    for area, q, v in quantities:
        t.add_initial_quantity(area, q, v)
    for axis, area, vals in borders:
        t.add_border_condition(0, axis, area, vals)
    return t


def test_engine_launcher_task(H):
    """parseTaskCubicAcoustic (launcher/main.cpp:422-467): 2-D 100 x 50, bs 2,
    Courant 1, IsotropicMaterial(1, 1, 0), a PRESSURE sphere of radius 10 at
    (50, 25), PRESSURE = 0 on the y- face area; 10 steps."""
    quantities = [(("sphere", 10.0, (50.0, 25.0, 0.0)), "PRESSURE", 10.0)]
    borders = [(1, ("box", (-1e3, -1e3, -1e3), (1e3, 1e-5, 1e3)), {"PRESSURE": lambda t: 0.0})]
    ref = A.Engine(2, 2, [100, 50], [1.0, 1.0], 1.0, 1.0, 1.0, ic_quantities=quantities, borders=borders,
                   number_of_snaps=10)
    he = H.Engine(host_task(H, 2, 2, [100, 50], [1.0, 1.0], 1.0, (1.0, 1.0, 0.0), 10, quantities, borders))
    assert he.matrix_structure(0) == 3
    assert he.maximal_eigenvalue(0) == ref.b.maximal_eigenvalue == 1.0
    assert np.float64(he.time_step).tobytes() == np.float64(ref.time_step).tobytes()  # afterConstruction
    he.profile(0)
    ref.run()
    he.run()
    assert he.steps == ref.steps_done == 10
    assert np.float64(he.time_step).tobytes() == np.float64(ref.time_step).tobytes()
    assert he.last_path(0) == "generic"
    assert he.profile_kernels(0) == ["k_stage_generic"], he.profile_kernels(0)
    got = he.pde(0)
    assert got.shape == (104, 54, 3)
    want = ref.b.pde.reshape(got.shape)
    assert np.abs(want[2:-2, 2:-2, 2]).max() > 1.0
    # the whole layer, ghosts included: the face fills and the stages write memory
    # exactly where the reference's do (no one-pass step forms ghosts on the chip;
    # with two stages per step the y- fills land in the other layer)
    assert np.array_equal(got, want), f"{int((got != want).sum())} values differ"


@pytest.mark.parametrize("h,courant,instance", [((1.0, 1.0, 1.0), 1.0, "!KF0"), ((0.5, 0.4, 0.3), 0.9, "KF0")])
def test_engine_3d(H, h, courant, instance):
    """[24, 20, 18], a PRESSURE sphere, 6 steps on the one-pass step; Courant 1
    on h = 1 puts every foot on a node (q = 1: the !KF0 instance)."""
    sizes = [24, 20, 18]
    centre = tuple(0.5 * (n - 1) * hh for n, hh in zip(sizes, h))
    quantities = [(("sphere", 5.0 * min(h), centre), "PRESSURE", 10.0)]
    ref = A.Engine(3, 2, sizes, list(h), courant, RHO, LAM, ic_quantities=quantities, number_of_snaps=6)
    he = H.Engine(host_task(H, 3, 2, sizes, h, courant, (RHO, LAM, 0.0), 6, quantities))
    assert he.matrix_structure(0) == 3 and he.path(0) == "fused"
    assert np.float64(he.time_step).tobytes() == np.float64(ref.time_step).tobytes()  # afterConstruction
    kf = [math.floor(abs(C * (-ref.time_step)) / hh) for hh in h]
    assert (max(kf) == 0) == (instance == "KF0") and max(kf) < 2, kf
    he.profile(0)
    ref.run()
    he.run()
    assert he.steps == ref.steps_done == 6
    assert np.float64(he.time_step).tobytes() == np.float64(ref.time_step).tobytes()
    assert he.last_path(0) == "fused"
    assert he.profile_kernels(0) == [f"k_step_acoustic<2, 64, {instance}>"], he.profile_kernels(0)
    got = he.pde(0)
    want = ref.b.pde.reshape(got.shape)
    assert want[2:-2, 2:-2, 2:-2].any()
    assert np.array_equal(got, want), f"{int((got != want).sum())} values differ"
