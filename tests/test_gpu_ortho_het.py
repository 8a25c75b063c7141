"""Per-node orthotropic materials on the one-pass orthotropic step
(k_step_ortho<..., HET>, kernels_ortho.hip) and its dispatch, bitwise against
the oracle's stage sequence run with each material's orthotropic tables.  The
tables are the numpy restatement of tests/test_ortho_cpu.py, never the
product's.  Materials: MAT_A, MAT_B and MAT_A turned by 90 degrees about z (the
other ply of a cross-ply laminate).  Unless stated otherwise a case takes a
random state on the inner nodes with zero ghosts, random ids, tau at Courant
0.9 on the largest eigenvalue of all materials (floor(q) = 0 everywhere) and
runs 3 steps in the exact build (conftest)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import (assert_same, assert_same_inner, context_for, oracle_body, random_materials,
                           random_state, tables)
from tests.test_ortho_cpu import MAT_A, MAT_B, max_eigenvalue, ortho_tables
from tests.test_ortho_het_cpu import hand_permutation

pytestmark = pytest.mark.gpu

H_A = (0.5, 0.4, 0.3)
PLY_A = (MAT_A[0], hand_permutation(MAT_A[1]))
MATS = (MAT_A, MAT_B, PLY_A)
# HET instances that are not built (ortho_het_built): borderSize
# >= 2 with rows longer than 512 nodes; those grids keep the generic stages
NOT_BUILT = lambda bs, sizes: bs >= 2 and sizes[2] > 512


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def scaled(mat, f):
    return (mat[0], tuple(v * f for v in mat[1]))


def het_body(bs, sizes, h=H_A, mats=MATS, ids="random", seed=5):
    """An oracle body whose stage takes each node's own orthotropic tables."""
    b = oracle_body(3, bs, sizes, h=h, materials=((4.0, 2.0, 1.0),) * len(mats))
    b.tables = [t if isinstance(t[0], np.ndarray) else ortho_tables(*t) for t in mats]
    b.maximal_eigenvalue = max(max_eigenvalue(t[2]) for t in b.tables)
    if ids == "random":
        random_materials(b, seed=seed)
    elif ids is not None:
        its = b.inner_indices()
        b.mat_id[b.flat_index(its)] = np.asarray(ids(its), dtype=np.uint8)
    return b


def courant_tau(b, courant=0.9):
    return courant * min(b.h[:3]) / b.maximal_eigenvalue


def oracle_step(b, tau):
    for s in range(3):
        b.stage(s, tau)


def kernel_names(ctx):
    return [v["kernel"] for v in ctx.profile_read().values() if v["launches"] > 0]


def assert_het_kernel(names, bs=None, zt=None, fma=False):
    assert names and all(n.startswith("k_step_ortho<") and "HET" in n for n in names), names
    if bs is not None:
        assert names == [f"k_step_ortho<{bs}, {zt}, KF0, HET{', FMA' if fma else ''}>"], names


def run_case(b, tau=None, steps=3, setup=None, seed=None, expect="fused"):
    """`steps` steps of a context for `b` against the oracle, bitwise; returns the kernels run."""
    random_state(b, seed=sum(b.sizes) + b.bs if seed is None else seed, ghosts=False)
    ctx = context_for(b)
    if setup is not None:
        setup(ctx)
    if expect == "fused":
        assert ctx.matrix_structure() == 2
    tau = courant_tau(b) if tau is None else tau
    ctx.profile(True)
    for step in range(steps):
        oracle_step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == expect, f"step {step} ran {ctx.last_path}"
        assert_same(ctx, b, f"ortho HET bs {b.bs} {b.sizes} step {step}")
    names = kernel_names(ctx)
    ctx.close()
    if expect == "fused":
        assert_het_kernel(names)
    else:
        assert names and all(n == "k_stage_generic" for n in names), names
    return names


# ------------------------------------------------------------------ shapes --

@pytest.mark.parametrize("sizes,bs", [([6, 9, 37], 2),    # ZT 64 with idle lanes
                                      ([4, 5, 64], 2),    # no idle lane
                                      ([4, 5, 65], 2),    # two waves: ids across the wave seam
                                      ([4, 2, 4], 2),     # the minimum: Y = bs, Z = 2 bs
                                      ([6, 9, 37], 1),
                                      ([5, 7, 20], 3),
                                      ([3, 4, 515], 2)])  # not built: the generic stages, same bits
def test_shapes(G, sizes, bs):
    b = het_body(bs, sizes)
    if NOT_BUILT(bs, sizes):
        ctx = context_for(b)
        assert ctx.matrix_structure() == 2 and ctx.effective_path == "generic"
        ctx.close()
        run_case(b, expect="generic")
        return
    names = run_case(b)
    zt = next(t for t in (64, 128, 256, 512, 1024) if sizes[2] <= t)
    assert_het_kernel(names, bs, zt)


def test_long_rows_at_border_size_1(G):
    """The one 1024-thread HET instance that fits its 128 VGPRs."""
    names = run_case(het_body(1, [3, 4, 515]), steps=2)
    assert_het_kernel(names, 1, 1024)


# -------------------------------------------------------- layer interfaces --

X, Y, Z = 6, 9, 37
LAYOUTS = {
    "x": lambda its: its[:, 0] >= X // 2,
    "y": lambda its: its[:, 1] >= Y // 2,
    "z": lambda its: its[:, 2] >= Z // 2,
    "node": lambda its: (its[:, 0] == 3) & (its[:, 1] == 4) & (its[:, 2] == 17),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layer_interfaces(G, layout):
    """Two materials split at X/2, Y/2, Z/2, and one material at a single
    interior node: an id from the wrong row of the ring, the wrong plane or a
    neighbour's lane changes the bits."""
    b = het_body(2, [X, Y, Z], mats=(MAT_A, PLY_A), ids=LAYOUTS[layout])
    inner_ids = b.mat_id[b.flat_index(b.inner_indices())]
    assert 0 < int(inner_ids.sum()) < len(inner_ids)
    assert_het_kernel(run_case(b), 2, 64)


# -------------------------------------------------------------- chunk seams --

@pytest.mark.parametrize("rows", [4, 1])
def test_chunk_seams(G, rows):
    """Partial last chunk: the prologue's ids at both edges of every chunk, the
    id row clamped at Y - 1 in every chunk that reaches the plane's end."""
    run_case(het_body(2, [6, 9, 37]), setup=lambda c: c.set_schedule(G.SCHED_SINGLE, rows_per_block=rows))


# ----------------------------------------------------- material table edges --

def test_32_materials_run_fused_33_generic(G):
    for n, expect in ((32, "fused"), (33, "generic")):
        mats = tuple(scaled(MAT_A, 1 + 0.01 * k) for k in range(n))
        b = het_body(2, [4, 5, 64], mats=mats)
        assert len(np.unique(b.mat_id)) == n
        run_case(b, expect=expect)


def test_one_material_with_ids(G):
    b = het_body(2, [4, 5, 64], mats=(MAT_A,), ids=None)
    random_state(b, seed=3, ghosts=False)
    ctx = context_for(b)
    ctx.set_material_ids(b.mat_id)  # all zero
    assert ctx.matrix_structure() == 2
    tau = courant_tau(b)
    ctx.profile(True)
    for step in range(3):
        oracle_step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == "fused"
        assert_same(ctx, b, f"one material, ids set, step {step}")
    assert_het_kernel(kernel_names(ctx), 2, 64)
    ctx.close()


def test_mixed_isotropic_and_orthotropic_set_stays_general(G):
    iso = O.isotropic_elastic_matrices(3, 4.0, 2.0, 1.0)
    b = het_body(2, [4, 5, 64], mats=(iso, MAT_A))
    ctx = context_for(b)
    assert ctx.matrix_structure() == 0 and ctx.effective_path == "generic"
    ctx.close()
    run_case(b, expect="generic")


def test_call_order_of_ids_and_materials(G):
    """gcmx_set_material_ids before gcmx_set_materials and the reverse: the same dispatch."""
    b = het_body(2, [4, 5, 64])
    random_state(b, seed=4, ghosts=False)
    tau = courant_tau(b)
    U, U1, L = tables(b)
    ctxs = []
    for ids_first in (True, False):
        c = G.Context(3, 2, [4, 5, 64], h=list(H_A))
        if ids_first:
            c.set_material_ids(b.mat_id)
            c.set_materials(U, U1, L)
        else:
            c.set_materials(U, U1, L)
            assert c.matrix_structure() == 0  # three materials and no ids yet: general
            c.set_material_ids(b.mat_id)
        c.upload(b.pde)
        c.profile(True)
        ctxs.append(c)
    oracle_step(b, tau)
    for c in ctxs:
        assert c.matrix_structure() == 2 and c.effective_path == "fused"
        c.step(tau)
        assert c.last_path == "fused"
        assert_het_kernel(kernel_names(c), 2, 64)
        assert_same(c, b, "call order")
        c.close()


# ---------------------------------------------------------------- tau cases --

def test_floor_q_1_takes_the_stages_then_fused_again(G):
    """h = (1, 1, 1), tau 0.158: MAT_A's P pair has floor(q) = 1 on x (q = 1.499),
    no HET instance: the generic stages, equal bits; back at Courant 0.9 the
    one-pass step runs again."""
    b = het_body(2, [6, 9, 37], h=(1.0, 1.0, 1.0))
    L = b.tables[0][2]
    assert int(np.floor(abs(L[0, 4]) * 0.158)) == 1
    random_state(b, seed=21, ghosts=False)
    ctx = context_for(b)
    assert ctx.matrix_structure() == 2
    ctx.profile(True)
    for tau, expect in ((0.158, "generic"), (courant_tau(b), "fused"), (0.158, "generic"), (courant_tau(b), "fused")):
        oracle_step(b, tau)
        ctx.step(tau)
        assert ctx.last_path == expect, (tau, ctx.last_path)
        assert_same(ctx, b, f"tau {tau}")
    names = kernel_names(ctx)
    assert sorted(set(names)) == ["k_stage_generic", "k_step_ortho<2, 64, KF0, HET>"], names
    ctx.close()


# ---------------------------------------------------------------- fallbacks --

def test_faces_fall_back_to_the_stages(G):
    """gcmx_step_faces with a Vy / Syy condition on the y- face: the generic
    stages with per-node tables, inner nodes equal to the oracle."""
    from tests.test_gpu_faces import QCODE
    b = het_body(2, [6, 9, 37])
    random_state(b, seed=12, ghosts=False)
    tau = courant_tau(b)
    ctx = context_for(b)
    vals = {"Vy": 0.05, "Syy": -0.2}
    faces = [None, None, [(QCODE[q], vals[q]) for q in ("Vy", "Syy")], None, None, None]
    inner0 = np.array(b.inner_indices()[b.inner_indices()[:, 1] == 0])

    def fill_y_minus():  # BorderConditions::handleBorderPoint on the y- face
        for a in range(1, b.bs + 1):
            inn = inner0.copy(); inn[:, 1] += a
            gh = inner0.copy(); gh[:, 1] -= a
            fi, fg = b.flat_index(inn), b.flat_index(gh)
            g = b.pde[fi].copy()
            for q in ("Vy", "Syy"):
                j = O.quantity_index(3, q)
                g[:, j] = -b.pde[fi][:, j] + 2 * vals[q]
            b.pde[fg] = g

    for step in range(3):
        b.stage(0, tau)
        fill_y_minus()
        b.stage(1, tau)
        b.stage(2, tau)
        ctx.step_faces(tau, faces)
        assert ctx.last_path == "generic"
        assert_same_inner(ctx, b, f"faces step {step}")
    assert ctx.effective_path == "generic"
    ctx.close()


def test_step_ode_is_step_then_ode(G):
    tau0 = [0.3, 0.5, 0.7]
    b = het_body(2, [6, 9, 37])
    random_state(b, seed=15, ghosts=False)
    tau = courant_tau(b)
    a, c = context_for(b), context_for(b)
    c.profile(True)
    for _ in range(3):
        a.step(tau)
        a.ode_maxwell(tau, tau0)
        c.step_ode(tau, tau0)
        assert not c.last_ode_fused and c.last_path == "fused"
    assert np.array_equal(a.download(), c.download())
    assert any("HET" in n for n in kernel_names(c))
    b.odes, b.tau0 = ["MAXWELL_VISCOSITY"], tau0
    for _ in range(3):
        oracle_step(b, tau)
        b.apply_odes(tau)
    assert_same(c, b, "step_ode")
    a.close(); c.close()


# ------------------------------------------------------------------- layout --

def test_padded_layout(G, monkeypatch):
    """Strides that the sizes do not imply; the id array stays unpadded."""
    for k, v in {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"}.items():
        monkeypatch.setenv(k, v)
    names = run_case(het_body(2, [6, 9, 37]), seed=17)
    assert_het_kernel(names, 2, 64)
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
    """16 x 6 x 20 as 8 + 8 planes, each slab with its own inner nodes' ids."""
    X, Y, Z, bs, seed, steps = 16, 6, 20, 2, 0x5EED, 3
    b = het_body(bs, [X, Y, Z])
    U, U1, L = tables(b)
    b.pde[:] = 0.0
    O.fill_random(b, [X, Y, Z], seed)
    tau = courant_tau(b)
    ids_all = b.mat_id.reshape(X + 2 * bs, Y + 2 * bs, Z + 2 * bs)
    sc = {"bfirst": G.SCHED_BFIRST, "xslab": G.SCHED_XSLAB}[sched]
    slabs = []
    for x0 in (0, 8):
        c = G.Context(3, bs, [8, Y, Z], start=[x0, 0, 0], h=list(H_A))
        c.set_materials(U, U1, L)
        c.set_material_ids(np.ascontiguousarray(ids_all[x0:x0 + 8 + 2 * bs]))
        c.fill_random([X, Y, Z], seed)
        c.set_schedule(sc)
        c.profile(True)
        slabs.append(c)
    G.comm_init_local(slabs)
    whole = G.Context(3, bs, [X, Y, Z], h=list(H_A))
    whole.set_materials(U, U1, L)
    whole.set_material_ids(b.mat_id)
    whole.fill_random([X, Y, Z], seed)
    G.local_group_steps(slabs, tau, steps)
    for _ in range(steps):
        whole.step(tau)
        oracle_step(b, tau)
    assert all(c.matrix_structure() == 2 and c.last_path == "fused" for c in slabs + [whole])
    for c in slabs:
        names = {n for n in kernel_names(c) if n}  # the halo copies carry no kernel name
        assert names == {"k_step_ortho<2, 64, KF0, HET>"}, names

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
    b = het_body(2, [8, 9, 37])
    random_state(b, seed=18, ghosts=False)
    tau = courant_tau(b)
    ex, fm = context_for(b), context_for(b)
    fm.fp_mode = G.FP_FMA
    assert ex.fp_mode == G.FP_EXACT and fm.fp_mode == G.FP_FMA
    fm.profile(True)
    for _ in range(20):
        ex.step(tau)
        fm.step(tau)
    names = kernel_names(fm)
    assert names == ["k_step_ortho<2, 64, KF0, HET, FMA>"] and "HET, FMA" in names[0], names
    want, got = ex.download(), fm.download()
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"HET FMA build vs exact build after 20 steps: relative L2 {rel:.3e}")
    assert rel <= 1e-10, rel
    ex.close(); fm.close()


# ------------------------------------------------------------------ engine --

PLY_B = (MAT_B[0], hand_permutation(MAT_B[1]))


def test_engine_cross_ply_body(G):
    """One ORTHOTROPIC body 24 x 12 x 20 (the launcher task's box and pressure
    sphere on a coarser grid): MAT_B below y = 1, its 90-degree ply above, through
    the Python Task / Engine binding.  Same step count, tau bits and final state
    as the oracle engine run with both tables and the same ids, on the one-pass step."""
    from gcm_amd import _gcm_host as H
    sizes, h = [24, 12, 20], [4.0 / 23, 2.0 / 11, 1.0 / 19]
    sphere = (("sphere", 0.5, (2.0, 1.0, 0.5)), "PRESSURE", 10.0)
    box = ("box", (-1.0, 1.0, -1.0), (10.0, 10.0, 10.0))
    ot = O.Task(D=3, border_size=2, h=h, cubics={0: (sizes, [0, 0, 0])}, courant=1.0,
                default_material=O.Material(4.0, 2.0, 1.0), inhomogeneities=[(box, O.Material(4.0, 2.0, 1.0))],
                number_of_snaps=5, ic_quantities=[sphere])
    oe = O.Engine(ot)
    ob = oe.bodies[0]
    inner_ids = ob.mat_id[ob.flat_index(ob.inner_indices())].reshape(sizes)
    assert np.all(inner_ids[:, :6] == 0) and np.all(inner_ids[:, 6:] == 1)
    ob.tables = [ortho_tables(*MAT_B), ortho_tables(*PLY_B)]
    ob.maximal_eigenvalue = max(max_eigenvalue(t[2]) for t in ob.tables)
    oe.time_step = oe.estimate_time_step()
    oe.required_time = oe.time_step * ot.number_of_snaps * ot.steps_per_snap
    for _, _, L in ob.tables:
        assert all(int(np.floor(abs(L[s, k]) * oe.time_step / h[s])) == 0 for s in range(3) for k in range(9))

    t = H.Task()
    t.dimensionality = 3
    t.border_size = 2
    t.h = h
    t.courant = 1.0
    t.number_of_snaps = 5
    t.add_body(0, sizes, [0, 0, 0])
    t.set_default_orthotropic_material(MAT_B[0], list(MAT_B[1]))
    t.add_orthotropic_material(box, PLY_B[0], list(PLY_B[1]))
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


def test_engine_stack_of_two_orthotropic_bodies(G, monkeypatch):
    """Two orthotropic bodies of different materials in y contact run as one
    grid with a two-material table on the one-pass step; GCMX_NO_STACKS=1
    (separate bodies, per-stage copies) gives the same inner nodes."""
    from gcm_amd import _gcm_host as H

    def task():
        t = H.Task()
        t.dimensionality = 3
        t.border_size = 2
        t.h = [1.0, 1.0, 1.0]
        t.courant = 0.9
        t.number_of_snaps = 5
        t.add_body(0, [10, 7, 64], [0, 0, 0])
        t.add_body(1, [10, 5, 64], [0, 7, 0])
        t.set_body_orthotropic_material(0, MAT_B[0], list(MAT_B[1]))
        t.set_body_orthotropic_material(1, PLY_B[0], list(PLY_B[1]))
        t.add_initial_quantity(("sphere", 5.0, (5.0, 5.5, 32.0)), "PRESSURE", 10.0)
        return t

    def inner(a):
        return a[2:-2, 2:-2, 2:-2]

    he = H.Engine(task())
    assert all(he.matrix_structure(i) == 2 and he.path(i) == "fused" for i in range(2))
    he.run()
    assert all(he.last_path(i) == "fused" for i in range(2))
    monkeypatch.setenv("GCMX_NO_STACKS", "1")
    sep = H.Engine(task())
    sep.run()
    assert sep.steps == he.steps and sep.last_path(0) == "generic"
    for i in range(2):
        got, want = inner(he.pde(i)), inner(sep.pde(i))
        assert np.any(want != 0.0)
        assert np.array_equal(got, want), f"body {i}: {int((got != want).sum())} differ"
