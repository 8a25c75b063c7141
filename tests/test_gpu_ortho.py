"""The one-pass orthotropic step (k_step_ortho, kernels_ortho.hip) and its
dispatch, bitwise against the oracle's stage sequence run with orthotropic
tables.  The tables are the numpy restatement of
ElasticModel<3>::constructNotRotated in tests/test_ortho_cpu.py, never the
product's.  Unless stated otherwise a case takes a random state on the inner
nodes with zero ghosts and runs 3 steps in the exact build (conftest)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_same, assert_same_inner, context_for, oracle_body, random_state
from tests.test_ortho_cpu import MAT_A, MAT_B, max_eigenvalue, ortho_tables

pytestmark = pytest.mark.gpu

H_A = (0.5, 0.4, 0.3)
ERR_CFL = 2  # GCMX_ERR_CFL


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def ortho_body(bs, sizes, h=H_A, mat=MAT_A):
    """An oracle body whose stage runs the orthotropic tables of `mat`."""
    b = oracle_body(3, bs, sizes, h=h)
    b.tables = [ortho_tables(*mat)]
    b.maximal_eigenvalue = max_eigenvalue(b.tables[0][2])
    return b


def courant_tau(b, courant=0.9):
    return courant * min(b.h[:3]) / b.maximal_eigenvalue


def oracle_step(b, tau):
    for s in range(3):
        b.stage(s, tau)


def kernel_names(ctx):
    return [v["kernel"] for v in ctx.profile_read().values() if v["launches"] > 0]


def run_case(bs, sizes, h=H_A, tau=None, steps=3, setup=None, seed=None):
    b = ortho_body(bs, sizes, h)
    random_state(b, seed=sum(sizes) + bs if seed is None else seed, ghosts=False)
    ctx = context_for(b)
    if setup is not None:
        setup(ctx)
    tau = courant_tau(b) if tau is None else tau
    ctx.profile(True)
    for step in range(steps):
        oracle_step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == "fused", f"step {step} ran {ctx.last_path}"
        assert_same(ctx, b, f"ortho bs {bs} {sizes} step {step}")
    names = kernel_names(ctx)
    ctx.close()
    return names


# ------------------------------------------------------------ recognition --

def test_recognition(G):
    b = ortho_body(2, [6, 9, 37])
    ctx = context_for(b)
    assert ctx.matrix_structure() == 2
    assert ctx.effective_path == "fused"
    ctx.profile(True)
    random_state(b, seed=1, ghosts=False)
    ctx.upload(b.pde)
    ctx.step(courant_tau(b))
    assert ctx.last_path == "fused"
    names = kernel_names(ctx)
    assert names and all(n.startswith("k_step_ortho<") for n in names), names
    ctx.close()

    iso = oracle_body(3, 2, [6, 9, 37])
    ctx = context_for(iso)
    assert ctx.matrix_structure() == 1
    ctx.close()

    U, U1, L = (a.copy() for a in ortho_tables(*MAT_A))
    assert U[1, 6, 0] == 0.0
    U[1, 6, 0] = 1e-3  # one structural zero
    b.tables = [(U, U1, L)]
    ctx = context_for(b)
    assert ctx.matrix_structure() == 0
    assert ctx.effective_path == "generic"
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
    zt = next(t for t in (64, 128, 256, 512, 1024) if sizes[2] <= t)
    assert names == [f"k_step_ortho<{bs}, {zt}, KF0>"], names


@pytest.mark.parametrize("rows", [4, 1])
def test_chunk_seams(G, rows):
    """Partial last chunk, a prologue at both edges of every chunk."""
    run_case(2, [6, 9, 37], setup=lambda c: c.set_schedule(G.SCHED_SINGLE, rows_per_block=rows))


# ---------------------------------------------------------- mixed floor(q) --

@pytest.mark.parametrize("sizes,bs,h,tau", [([6, 9, 37], 2, (1.0, 1.0, 1.0), 0.158),
                                            ([5, 4, 6], 3, H_A, 0.12)])
def test_mixed_floor_q(G, sizes, bs, h, tau):
    """The KF0 = false instance: the P pair's foot beyond the first interval
    (q = 1.499 / 1.060 / 0.749 on x / y / z; bs 3: 2.28 / 2.01 / 1.90) while the
    shear pairs stay below it."""
    L = ortho_tables(*MAT_A)[2]
    kf = [[int(np.floor(abs(L[s, 2 * p]) * tau / h[s])) for p in range(3)] for s in range(3)]
    assert max(max(r) for r in kf) >= 1 and min(min(r) for r in kf) == 0
    names = run_case(bs, sizes, h=h, tau=tau)
    zt = 64
    assert names == [f"k_step_ortho<{bs}, {zt}, !KF0>"], names


def test_courant_too_large_is_refused(G):
    b = ortho_body(2, [6, 9, 37], h=(1.0, 1.0, 1.0))
    ctx = context_for(b)
    with pytest.raises(G.GcmxError) as e:
        ctx.step(0.25)  # q = 2.37 >= borderSize
    assert e.value.status == ERR_CFL
    ctx.close()


# -------------------------------------------------------------- dispatch --

def test_paths_agree(G):
    """GENERIC, SPLIT and AUTO give identical bits; gcmx_stage x 3 == gcmx_step."""
    b = ortho_body(2, [6, 9, 37])
    random_state(b, seed=11, ghosts=False)
    tau = courant_tau(b)
    ctxs = {"auto": context_for(b), "generic": context_for(b, path=G.PATH_GENERIC),
            "split": context_for(b, path=G.PATH_SPLIT), "stages": context_for(b)}
    for _ in range(3):
        oracle_step(b, tau)
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


def test_faces_fall_back_to_the_stages(G):
    """gcmx_step_faces with a Vx / Sxx condition on the x- face: the generic
    stages, equal to the oracle; a later plain step stays on them (a face's
    ghosts were written)."""
    from tests.test_gpu_faces import QCODE
    b = ortho_body(2, [6, 9, 37])
    random_state(b, seed=12, ghosts=False)
    tau = courant_tau(b)
    ctx = context_for(b)
    vals = {"Vx": 0.05, "Sxx": -0.2}
    faces = [[(QCODE[q], vals[q]) for q in ("Vx", "Sxx")]] + [None] * 5
    inner0 = np.array(b.inner_indices()[b.inner_indices()[:, 0] == 0])

    def fill_x_minus():  # BorderConditions::handleBorderPoint on the x- face
        for a in range(1, b.bs + 1):
            inn = inner0.copy(); inn[:, 0] += a
            gh = inner0.copy(); gh[:, 0] -= a
            fi, fg = b.flat_index(inn), b.flat_index(gh)
            g = b.pde[fi].copy()
            for q in ("Vx", "Sxx"):
                j = O.quantity_index(3, q)
                g[:, j] = -b.pde[fi][:, j] + 2 * vals[q]
            b.pde[fg] = g

    for step in range(3):
        fill_x_minus()
        oracle_step(b, tau)
        ctx.step_faces(tau, faces)
        assert ctx.last_path == "generic"
        assert_same_inner(ctx, b, f"faces step {step}")
    assert ctx.effective_path == "generic"
    ctx.close()


def test_touched_ghost_falls_back_to_the_stages(G):
    """copy_box into the y+ ghost rows (a contact's copy): the generic stages from then on."""
    b = ortho_body(2, [6, 9, 37])
    other = ortho_body(2, [6, 9, 37])
    random_state(b, seed=13, ghosts=False)
    random_state(other, seed=14, ghosts=False)
    tau = courant_tau(b)
    ctx, src = context_for(b), context_for(other)
    X, Y, Z = b.sizes
    for step in range(2):
        ctx.copy_box([0, Y, 0], [X, Y + b.bs, Z], src, [0, 0, 0])
        b.pde[b.box_flat([0, Y, 0], [X - 1, Y + b.bs - 1, Z - 1])] = \
            other.pde[other.box_flat([0, 0, 0], [X - 1, b.bs - 1, Z - 1])]
        oracle_step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == "generic"
        assert_same_inner(ctx, b, f"copy_box step {step}")
    ctx.close(); src.close()


def test_step_ode_is_step_then_ode(G):
    b = ortho_body(2, [6, 9, 37])
    random_state(b, seed=15, ghosts=False)
    tau = courant_tau(b)
    a, c = context_for(b), context_for(b)
    for _ in range(3):
        a.step(tau)
        a.ode_maxwell(tau, [0.3])
        c.step_ode(tau, [0.3])
        assert not c.last_ode_fused and c.last_path == "fused"
    assert np.array_equal(a.download(), c.download())
    b.odes, b.tau0 = ["MAXWELL_VISCOSITY"], [0.3]
    for _ in range(3):
        oracle_step(b, tau)
        b.apply_odes(tau)
    assert_same(c, b, "step_ode")
    a.close(); c.close()


def test_border_size_3_long_rows_take_the_stages(G):
    """borderSize 3 with rows longer than 512 has no one-pass instance (a
    1024-thread block leaves 128 VGPRs): the generic stages, same bits."""
    b = ortho_body(3, [4, 4, 515])
    random_state(b, seed=16, ghosts=False)
    tau = courant_tau(b)
    ctx = context_for(b)
    assert ctx.matrix_structure() == 2 and ctx.effective_path == "generic"
    oracle_step(b, tau)
    ctx.step(tau)
    assert_same(ctx, b, "bs 3, Z 515")
    ctx.close()


def test_padded_layout(G, monkeypatch):
    """Strides that the sizes do not imply (the knobs of tests/test_gpu_layout.py)."""
    for k, v in {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"}.items():
        monkeypatch.setenv(k, v)
    names = run_case(2, [6, 9, 37], seed=17)
    assert names == ["k_step_ortho<2, 64, KF0>"]
    padded = G.Context(3, 2, [6, 9, 37], device=0)
    gp = padded.geometry()
    padded.close()
    monkeypatch.undo()
    plain = G.Context(3, 2, [6, 9, 37], device=0)
    g0 = plain.geometry()
    plain.close()
    assert gp["stride"][1] > g0["stride"][1] and gp["stride"][0] > g0["stride"][0]  # the knobs took effect


# ------------------------------------------------------------------ slabs --

@pytest.mark.parametrize("sched", ["bfirst", "xslab"])
def test_two_slabs_equal_whole_and_oracle(G, sched):
    X, Y, Z, bs, seed, steps = 16, 6, 20, 2, 0x5EED, 3
    U, U1, L = ortho_tables(*MAT_A)
    b = ortho_body(bs, [X, Y, Z])
    b.pde[:] = 0.0
    O.fill_random(b, [X, Y, Z], seed)
    tau = courant_tau(b)
    sc = {"bfirst": G.SCHED_BFIRST, "xslab": G.SCHED_XSLAB}[sched]
    slabs = []
    for x0 in (0, 8):
        c = G.Context(3, bs, [8, Y, Z], start=[x0, 0, 0], h=list(H_A))
        c.set_materials(U[None], U1[None], L[None])
        c.fill_random([X, Y, Z], seed)
        c.set_schedule(sc)
        slabs.append(c)
    G.comm_init_local(slabs)
    whole = G.Context(3, bs, [X, Y, Z], h=list(H_A))
    whole.set_materials(U[None], U1[None], L[None])
    whole.fill_random([X, Y, Z], seed)
    G.local_group_steps(slabs, tau, steps)
    for _ in range(steps):
        whole.step(tau)
        oracle_step(b, tau)
    assert all(c.matrix_structure() == 2 and c.last_path == "fused" for c in slabs + [whole])

    def inner(c):
        return c.download().reshape(tuple(s + 2 * bs for s in c.sizes) + (9,))[bs:-bs, bs:-bs, bs:-bs]
    got = np.concatenate([inner(c) for c in slabs], axis=0)
    assert np.array_equal(got, inner(whole))
    assert np.array_equal(got, b.inner_view())
    for c in slabs + [whole]:
        c.close()


# -------------------------------------------------------------- FMA build --

def test_fma_build_within_tolerance(G):
    """(8, 9, 37), bs 2, 20 steps in GCMX_FP_FMA against the exact build:
    relative L2 <= 1e-10 (the north-star bound of tests/test_gpu_fma.py)."""
    b = ortho_body(2, [8, 9, 37])
    random_state(b, seed=18, ghosts=False)
    tau = courant_tau(b)
    ex, fm = context_for(b), context_for(b)
    fm.fp_mode = G.FP_FMA
    assert ex.fp_mode == G.FP_EXACT and fm.fp_mode == G.FP_FMA
    fm.profile(True)
    for _ in range(20):
        ex.step(tau)
        fm.step(tau)
    assert kernel_names(fm) == ["k_step_ortho<2, 64, KF0, FMA>"]
    want, got = ex.download(), fm.download()
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"FMA build vs exact build after 20 steps: relative L2 {rel:.3e}")
    assert rel <= 1e-10, rel
    ex.close(); fm.close()


# ------------------------------------------------------------------ engine --

def test_engine_reference_task(G):
    """The reference's 3-D cubic launcher task (launcher/main.cpp:376-419) through
    the Python Task / Engine binding: same step count and tau bits as the oracle
    engine with the orthotropic tables, final state bitwise equal, on the
    one-pass kernel."""
    from gcm_amd import _gcm_host as H
    sizes, h = [100, 50, 20], [4.0 / 99, 2.0 / 49, 1.0 / 19]
    sphere = (("sphere", 0.2, (2.0, 1.0, 0.5)), "PRESSURE", 10.0)
    ot = O.Task(D=3, border_size=2, h=h, cubics={0: (sizes, [0, 0, 0])}, courant=1.0,
                default_material=O.Material(4.0, 2.0, 1.0), number_of_snaps=5, ic_quantities=[sphere])
    oe = O.Engine(ot)
    ob = oe.bodies[0]
    ob.tables = [ortho_tables(*MAT_B)]
    ob.maximal_eigenvalue = max_eigenvalue(ob.tables[0][2])
    oe.time_step = oe.estimate_time_step()
    oe.required_time = oe.time_step * ot.number_of_snaps * ot.steps_per_snap
    L = ob.tables[0][2]
    assert all(int(np.floor(abs(L[s, k]) * oe.time_step / h[s])) == 0 for s in range(3) for k in range(9))

    t = H.Task()
    t.dimensionality = 3
    t.border_size = 2
    t.h = h
    t.courant = 1.0
    t.number_of_snaps = 5
    t.add_body(0, sizes, [0, 0, 0])
    t.set_default_orthotropic_material(MAT_B[0], list(MAT_B[1]))
    t.add_initial_quantity(*sphere)
    he = H.Engine(t)
    assert he.matrix_structure(0) == 2 and he.path(0) == "fused"
    assert he.maximal_eigenvalue(0) == ob.maximal_eigenvalue

    oe.run()
    he.run()
    assert he.steps == oe.steps_done
    assert np.float64(he.time_step).tobytes() == np.float64(oe.time_step).tobytes()
    assert he.last_path(0) == "fused"
    got = he.pde(0)
    want = ob.pde.reshape(got.shape)
    assert np.any(want != 0.0)
    assert np.array_equal(got, want), f"{int((got != want).sum())} values differ"
