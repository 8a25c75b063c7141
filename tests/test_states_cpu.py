"""The structured states of tests/states.py on the oracle alone (no GPU): the
facts the GPU suites rest on, for every material set the launch catalogue uses.

  * one step of an impulse at the centre leaves exactly a 3^D footprint
    (floor(q) = 0 on every wave: each stage reaches one node either way);
  * the step commutes with a power-of-two scaling while nothing overflows or
    underflows: scaled(+-1000) stays finite and equals ldexp of the unscaled
    result bit for bit;
  * scaled(-1060) stays finite and every output is subnormal (or zero);
  * a NaN in one inner node spreads in one step to the (2 bs + 1)^3 box around
    it, clipped to the grid, in all components: the oracle forms 0 * NaN where
    the kernels skip a structural zero, so this box is the largest set a taint
    may reach on the GPU (tests/test_gpu_nonfinite.py); the acoustic medium's
    region is stated on its own;
  * the catalogue's ODE, face and face-map entries keep the scaling facts, and
    each differs from the same launch without its feature, so that a feature
    that silently does not run cannot pass;
  * the part-cut placements and the steps-zcut family exist exactly for rows
    longer than 512, and steps-zcut jumps on the cut in every component."""
import numpy as np
import pytest

from tests import states
from tests.launch_catalog import (BY_NAME, H_GP, H_GP2, H_GP_EQ, ISO_GP, MAP_64, MAP_1024, MATERIAL_SETS, TWINS,
                                  courant_tau, partial_body, scaled_areas)

SIZES = {3: ([6, 7, 16], [9, 9, 16]), 2: ([9, 16], [12, 21])}
# the acoustic set and then the general-position sets last: the cases before
# them keep their ids
LATE = ("acoustic", "iso_gp", "iso_gp_eq", "iso2d_gp")
CASES = [(name, tuple(sizes))
         for name in sorted(MATERIAL_SETS, key=lambda n: (LATE.index(n) + 1 if n in LATE else 0, n))
         for sizes in SIZES[2 if "2d" in name else 3]]
TINY = np.finfo(np.float64).tiny


def body_of(name, sizes, bs=2):
    make, tau = MATERIAL_SETS[name]
    b = make(bs, list(sizes))
    return b, tau(b)


def step(b, tau, n=1):
    for _ in range(n):
        for s in range(b.D):
            b.stage(s, tau)
    return b.pde.reshape(tuple(b.shape_all) + (b.M,)).copy()


@pytest.mark.parametrize("name,sizes", CASES)
def test_impulse_footprint(name, sizes):
    b, tau = body_of(name, sizes)
    node = states.impulse(b, "centre")
    out = step(b, tau)
    assert np.isfinite(out).all()
    hit = np.argwhere((out != 0.0).any(axis=-1)) - b.bs
    box = np.array([[c + d for c, d in zip(node, off)] for off in np.ndindex(*(3,) * b.D)]) - 1
    assert sorted(map(tuple, hit)) == sorted(map(tuple, box)), f"footprint {sorted(map(tuple, hit))}"


@pytest.mark.parametrize("name,sizes", CASES)
def test_power_of_two_scaling_commutes(name, sizes):
    b, tau = body_of(name, sizes)
    states.uniform(b)
    base = step(b, tau)
    for e in (1000, -1000):
        b, tau = body_of(name, sizes)
        states.scaled(b, e)
        out = step(b, tau)
        assert np.isfinite(out).all(), e
        assert np.array_equal(out.view(np.uint64), np.ldexp(base, e).view(np.uint64)), e


@pytest.mark.parametrize("name,sizes", CASES)
def test_subnormal_state_stays_subnormal(name, sizes):
    b, tau = body_of(name, sizes)
    states.scaled(b, -1060)
    assert (np.abs(b.pde) < TINY).all() and (b.inner_view() != 0.0).mean() > 0.99
    out = step(b, tau)
    assert np.isfinite(out).all()
    assert (np.abs(out) < TINY).all()
    assert (b.inner_view(out.reshape(b.pde.shape)) != 0.0).mean() > 0.99


@pytest.mark.parametrize("name", ["iso", "iso_het", "ortho", "ortho_het", "iso_gp"])
@pytest.mark.parametrize("variant", ["vx-nan", "s-nan"])
def test_nan_spreads_to_the_5_cube(name, variant):
    sizes = [6, 7, 16]
    b, tau = body_of(name, sizes)
    node = tuple(s // 2 for s in sizes)
    states.taint(b, node, variant)
    out = b.inner_view(step(b, tau).reshape(b.pde.shape))
    bad = ~np.isfinite(out)
    want = np.zeros(out.shape[:3], dtype=bool)
    want[tuple(slice(max(0, c - 2), c + 3) for c in node)] = True
    assert np.array_equal(bad.any(axis=-1), want)
    assert np.array_equal(bad.all(axis=-1), want), "not every component of the box is tainted"
    out2 = b.inner_view(step(b, tau).reshape(b.pde.shape))
    if name == "iso" and variant == "vx-nan":
        assert int((~np.isfinite(out2)).any(axis=-1).sum()) == 378  # 6 x 7 x 9: the box grown by 2


def test_nan_region_of_the_acoustic_medium():
    """A NaN in Vx or in the pressure: the x stage couples Vx and p and carries
    the other two velocities through as 0 * NaN + v, so after the three stages the
    whole (2 bs + 1)^3 box is tainted in all four components, as in the elastic
    media."""
    sizes = [6, 7, 16]
    for variant in ("vx-nan", "s-nan"):
        b, tau = body_of("acoustic", sizes)
        node = tuple(s // 2 for s in sizes)
        states.taint(b, node, variant)
        bad = ~np.isfinite(b.inner_view(step(b, tau).reshape(b.pde.shape)))
        want = np.zeros(bad.shape[:3], dtype=bool)
        want[tuple(slice(max(0, c - 2), c + 3) for c in node)] = True
        assert np.array_equal(bad.any(axis=-1), want), variant
        assert np.array_equal(bad.all(axis=-1), want), variant


# ---- the two isotropic media: what coincides on one and not on the other ------
#
# The homogeneous isotropic kernels keep six structural coefficients per axis
# (IsoAxis a, b, g, p1, p2, s: iso.hpp) next to the constants 0.5 and 1, and
# per axis and wave speed the Newton coefficients, Lagrange weights and
# floor(q) of q = |L| tau / h.  "iso", the medium of the parity suites, is
# (4, 2, 1) on unit steps; "iso_gp" is ISO_GP on H_GP (tests/launch_catalog.py).

SLOTS = ("a", "b", "g", "p1", "p2", "s")


def _sig(D, i, j):
    """Index of sigma(i, j) in the PDE vector (sig3 of iso.hpp, sig2 of kernels_2d.hip)."""
    i, j = min(i, j), max(i, j)
    return D + i * D - ((i - 1) * i) // 2 + j - i


def slot_positions(D, S):
    """For axis S: slot -> ("U" or "U1", row, column, sign) of every entry of U
    and U1 that iso_u / iso_u1 (iso2_u / iso2_u1 in 2-D) give that slot, the
    first of each being the entry the host extracts the slot from; and the
    entries of U1's node-only shear column that hold the constant 1."""
    if D == 3:
        t1, t2 = (1 if S == 0 else 0), (1 if S == 2 else 2)
        s1, s2 = (-1 if S == 0 else 1), (1 if S == 2 else -1)
        ss, st1, st2 = _sig(3, S, S), _sig(3, t1, S), _sig(3, t2, S)
        s11, s22, s12 = _sig(3, t1, t1), _sig(3, t2, t2), _sig(3, t1, t2)
        return {"a": [("U", 0, ss, 1), ("U", 1, ss, -1)],
                "b": [("U", 2, st1, s1), ("U", 3, st1, -s1), ("U", 4, st2, s2), ("U", 5, st2, -s2)],
                "g": [("U", 8, ss, 1)],
                "p1": [("U1", ss, 0, 1), ("U1", ss, 1, -1)],
                "p2": [("U1", s11, 0, 1), ("U1", s22, 0, 1), ("U1", s11, 1, -1), ("U1", s22, 1, -1)],
                "s": [("U1", st1, 2, s1), ("U1", st1, 3, -s1), ("U1", st2, 4, s2), ("U1", st2, 5, -s2)],
                "one": [("U1", s12, 6, s1 * s2)]}
    t, s1 = 1 - S, (-1 if S == 0 else 1)
    ss, st, tt = _sig(2, S, S), _sig(2, t, S), _sig(2, t, t)
    return {"a": [("U", 0, ss, 1), ("U", 1, ss, -1)], "b": [("U", 2, st, s1), ("U", 3, st, -s1)],
            "g": [("U", 4, ss, 1)], "p1": [("U1", ss, 0, 1), ("U1", ss, 1, -1)],
            "p2": [("U1", tt, 0, 1), ("U1", tt, 1, -1)], "s": [("U1", st, 2, s1), ("U1", st, 3, -s1)],
            "one": [("U1", tt, 4, 1)]}


def slots_of(b, S):
    """The six slot values of axis S from the oracle's tables, every entry of a
    slot checked against the first (and the constant-1 entries against 1)."""
    U, U1, _ = b.tables[0]
    mats, out = {"U": U[S], "U1": U1[S]}, {}
    for slot, where in slot_positions(b.D, S).items():
        m, r, c, sign = where[0]
        v = sign * mats[m][r, c]
        for m, r, c, sign in where:
            assert mats[m][r, c] == sign * v, (slot, m, r, c)
        out[slot] = v
    assert out.pop("one") == 1.0
    return out


def q_of(b, tau):
    """Per axis (q of the P waves, q of the S waves), as build_tables forms them."""
    L = b.tables[0][2]
    return [tuple(abs(L[s][k] * (-tau)) / b.h[s] for k in (0, 2)) for s in range(b.D)]


def distinct(values):
    return len(set(values)) == len(values)


@pytest.mark.parametrize("name", ["iso_gp", "iso_gp_eq", "iso2d_gp"])
def test_the_general_medium_is_in_general_position(name):
    """No structural coefficient equals another, 0.5 or 1 or is a power of two, so
    a kernel that takes one slot or constant for another, or drops a factor,
    changes the result; and every product of the transform rounds."""
    D = 2 if "2d" in name else 3
    b, tau = body_of(name, SIZES[D][0])
    per_axis = [slots_of(b, S) for S in range(D)]
    for v in per_axis:
        assert v == per_axis[0]  # the structure belongs to the material, not to the axis
        mags = [abs(v[k]) for k in SLOTS]
        assert distinct(mags), v
        assert not set(mags) & {0.5, 1.0}, v
        assert all(np.frexp(m)[0] != 0.5 for m in mags), v
    q = q_of(b, tau)
    flat = [x for pair in q for x in pair]
    assert all(0.0 < x < 1.0 for x in flat), q
    q15 = q_of(b, courant_tau(b, 1.5))
    floors = [tuple(int(np.floor(x)) for x in pair) for pair in q15]
    if name == "iso_gp":
        assert distinct(flat), q
        assert np.allclose(q, [(0.643, 0.288), (0.9, 0.403), (0.409, 0.183)], atol=1e-3), q
        assert floors == [(1, 0), (1, 0), (0, 0)], floors
    elif name == "iso2d_gp":
        assert distinct(flat), q
        assert floors == [(1, 0), (0, 0)], floors  # the axes' P floors differ: gp-2d-iso-mixed-bs2-21x70
    else:  # equal steps: the medium of the instances that read one table for all three stages
        assert q[0] == q[1] == q[2] and distinct(q[0]), q
        assert floors == [(1, 0)] * 3, floors


@pytest.mark.parametrize("name", ["iso", "iso2d"])
def test_the_dyadic_medium_and_what_coincides_on_it(name):
    """The blind spot of the suites that run on (4, 2, 1) alone, on record: four
    slots have the magnitude of a constant of the kernels (|b| = 0.5; g = p2 = s
    = -1; in 2-D g = -0.5), all six are powers of two (every product u * v is exact, so the
    contracted row sums round like the exact ones), and on unit steps the three
    axes have the same q, hence bitwise the same table."""
    D = 2 if "2d" in name else 3
    b, tau = body_of(name, SIZES[D][0])
    for S in range(D):
        assert slots_of(b, S) == {"a": -0.25, "b": -0.5, "g": -1.0 if D == 3 else -0.5, "p1": -2.0, "p2": -1.0,
                                  "s": -1.0}
    q = q_of(b, tau)
    if D == 3:
        assert q == [(0.9, 0.45)] * 3
        assert [tuple(int(np.floor(x)) for x in pair) for pair in q_of(b, 1.5)] == [(1, 0)] * 3
    else:  # steps (1, 0.5): the 2-D axes do differ
        assert q == [(0.45, 0.225), (0.9, 0.45)]


def mutated(b, which):
    """`b`'s tables as a plausibly wrong kernel would effectively use them."""
    U, U1, L = (x.copy() for x in b.tables[0])
    mats = {"U": U, "U1": U1}
    for S in range(b.D):
        pos, v = slot_positions(b.D, S), slots_of(b, S)
        keep = lambda mag, like: float(np.copysign(mag, like))
        put = {"p2<->s": [("p2", v["s"]), ("s", v["p2"])],  # kS where iso_u1 needs kP2, and back
               "|b|=0.5": [("b", keep(0.5, v["b"]))],       # the magnitude of kHalf for kB's
               "|g|=1": [("g", keep(1.0, v["g"]))],         # the factor |g| dropped
               "one=|p2|": [("one", abs(v["p2"]))],         # |p2| where U1's shear column has 1
               "b=0.5": [("b", 0.5)],                       # kHalf for kB, the sign lost with it
               "one=p2": [("one", v["p2"])]}[which]         # kP2 for that 1, with p2's sign
        for slot, value in put:
            for m, r, c, sign in pos[slot]:
                mats[m][S][r, c] = sign * value
    return [(U, U1, L)]


# mutant -> one step on (4, 2, 1) keeps its bits.  The last two change a sign
# there (b = -0.5, p2 = -1), so the dyadic medium does show them: a wrong slot
# is hidden only where value AND sign coincide.
MUTANTS = {"p2<->s": True, "|b|=0.5": True, "|g|=1": True, "one=|p2|": True, "b=0.5": False, "one=p2": False}


@pytest.mark.parametrize("which", sorted(MUTANTS))
@pytest.mark.parametrize("D", [3, 2])
def test_a_wrong_coefficient_shows_on_the_general_medium_only(D, which):
    """One oracle step of the random state on mutated tables: bit-identical to
    the unmutated step on (4, 2, 1) where the exchanged values coincide (MUTANTS),
    and different on ISO_GP.  A GPU suite on the first medium alone cannot tell
    such a kernel from a right one."""
    out = {}
    for name in (("iso", "iso_gp", "iso_gp_eq") if D == 3 else ("iso2d", "iso2d_gp")):
        res = []
        for mutate in (False, True):
            b, tau = body_of(name, SIZES[D][0])
            if mutate:
                b.tables = mutated(b, which)
            states.uniform(b)
            res.append(step(b, tau))
        out[name] = np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64))
    hidden = MUTANTS[which] and not (D == 2 and which == "|g|=1")  # in 2-D g = -0.5 on (4, 2, 1)
    assert out.pop("iso" if D == 3 else "iso2d") == hidden, f"{which}: on the dyadic medium"
    assert not any(out.values()), f"{which}: {out}"


@pytest.mark.parametrize("conds,sizes,h", [(MAP_64, [6, 12, 64], H_GP), (MAP_1024, [4, 10, 1024], H_GP_EQ),
                                           (MAP_1024, [4, 10, 1024], H_GP)], ids=["map64", "map1024-eq", "map1024"])
def test_scaled_map_areas_select_the_unit_step_node_sets(conds, sizes, h):
    unit = partial_body(2, sizes, conds)
    gp = partial_body(2, sizes, scaled_areas(conds, h), materials=(ISO_GP,), h=h)
    assert len(unit.border) == len(gp.border) == len(conds)
    for (d, left, right, _), (d2, left2, right2, _) in zip(unit.border, gp.border):
        assert d == d2 and np.array_equal(left, left2) and np.array_equal(right, right2)
        n, face = len(left) + len(right), int(np.prod(sizes)) // sizes[d]
        assert 0 < n < 2 * face  # a part of the faces, as on unit steps


def test_the_twins_keep_shape_and_instance_and_take_the_general_medium():
    """A twin is its original on the other medium: same kind, grid and expected
    instance.  Unequal steps wherever the instance admits them: equal steps
    exactly for the entries marked UNI or ZS."""
    assert len(TWINS) == 24
    for twin, orig in TWINS.items():
        t, o = BY_NAME[twin], BY_NAME[orig]
        tb, ob = t.body(), o.body()
        assert (t.kind, t.prefix, t.marks, t.absent, t.fma_tag, t.compare, t.tau0, t.path, t.expect_path) == \
               (o.kind, o.prefix, o.marks, o.absent, o.fma_tag, o.compare, o.tau0, o.path, o.expect_path), twin
        assert (tb.D, tb.bs, tb.sizes, tb.start) == (ob.D, ob.bs, ob.sizes, ob.start), twin
        assert len(tb.border) == len(ob.border), twin
        want = body_of("iso2d_gp" if tb.D == 2 else "iso_gp", [8] * tb.D)[0]
        assert all(np.array_equal(x, y) for x, y in zip(tb.tables[0], want.tables[0])) and len(tb.tables) == 1, twin
        equal_axes = any(m in (", UNI", ", ZS") for m in t.marks)
        assert tuple(tb.h[:tb.D]) == (H_GP2 if tb.D == 2 else H_GP_EQ if equal_axes else H_GP), twin
        courant = 1.5 if "courant15" in twin else 0.9
        assert t.tau(tb) == courant_tau(tb, courant), twin
    for twin, widths in (("gp-slabs-bfirst-bs2-7+9x6x64", (7, 9)),):
        assert BY_NAME[twin].slabs == widths and widths[0] % 2 == 1 and tuple(BY_NAME[twin].body().h) == H_GP
    mixed = BY_NAME["gp-2d-iso-mixed-bs2-21x70"]
    assert mixed.tau(mixed.body()) == courant_tau(mixed.body(), 1.5) and tuple(mixed.body().h[:2]) == H_GP2


# ---- the catalogue's ODE, face and face-map entries, on the oracle alone ------

FEATURE_ENTRIES = ("tx2-faces-ode-bs2-4x8x64", "tx2-zs-faces-free6-bs2-4x12x1024", "tx2-map-bs2-6x12x64",
                   "gp-tx2-faces-ode-bs2-4x8x64", "gp-tx2-map-bs2-6x12x64")


def oracle_steps(entry, fill, n=2, body=None):
    b = entry.body() if body is None else body
    fill(b)
    t = 0.0
    for _ in range(n):
        out = entry.oracle_step(b, t)[-1]
        t += entry.tau(b)
    return out


@pytest.mark.parametrize("name", FEATURE_ENTRIES)
def test_feature_entries_commute_with_power_of_two_scaling(name):
    """The ODE factor is one more multiply and a mirrored ghost is a copy or a
    sign flip (every prescribed value is 0): the scaling argument holds."""
    entry = BY_NAME[name]
    base = oracle_steps(entry, states.uniform)
    for e in (1000, -1000):
        out = oracle_steps(entry, lambda b: states.scaled(b, e))
        assert np.isfinite(out).all(), e
        assert np.array_equal(out.view(np.uint64), np.ldexp(base, e).view(np.uint64)), e
    out = oracle_steps(entry, lambda b: states.scaled(b, -1060))
    assert np.isfinite(out).all()
    assert (np.abs(out) < TINY).all() and (out != 0.0).mean() > 0.99


def differing(a, b):
    return np.argwhere((a != b).any(axis=-1))


def test_the_ode_entries_differ_from_the_step_alone():
    for name in ("tx2-ode-bs2-4x6x64", "tx2-het-ode-bs1-5x7x64", "tx2-faces-ode-bs2-4x8x64",
                 "tx2-zs-ode-bs2-4x12x1024", "gp-tx2-ode-bs2-4x6x64", "gp-tx2-faces-ode-bs2-4x8x64"):
        entry = BY_NAME[name]
        plain = entry.body()
        states.uniform(plain)
        for k in range(2):  # the entry's two steps with Body.apply_odes left out
            for s in range(3):
                if entry.has_faces:
                    plain.apply_border(s, k * entry.tau(plain))
                plain.stage(s, entry.tau(plain))
        a, b = oracle_steps(entry, states.uniform), entry.grid(plain, plain.pde)
        assert (a[..., plain.D:] != b[..., plain.D:]).mean() > 0.99, name  # the stresses, two factors deep
    # two materials: the two factors differ, so ids cannot be ignored either
    het = BY_NAME["tx2-het-ode-bs1-5x7x64"]
    one = het.body()
    one.tau0 = [one.tau0[0]] * 2
    assert len(differing(oracle_steps(het, states.uniform), oracle_steps(het, states.uniform, body=one))) > 0


def test_the_map_entries_differ_from_whole_faces_and_from_no_faces():
    for name, conds in (("tx2-map-bs2-6x12x64", MAP_64), ("tx2-map-zs-bs2-4x10x1024", MAP_1024),
                        ("gp-tx2-map-bs2-6x12x64", MAP_64)):
        entry = BY_NAME[name]
        b0 = entry.body()
        got = oracle_steps(entry, states.uniform)
        everywhere = ("box", (-1e6,) * 3, (1e6,) * 3)  # partial_body cuts it to the condition's face
        gp = dict(materials=(ISO_GP,), h=b0.h) if name.startswith("gp-") else {}
        whole = partial_body(b0.bs, b0.sizes, [(a, s, everywhere, v) for a, s, _, v in conds], **gp)
        none = entry.body()
        none.border = []
        assert len(differing(got, oracle_steps(entry, states.uniform, body=whole))) > 0, name
        assert len(differing(got, oracle_steps(entry, states.uniform, body=none))) > 0, name


def test_the_zs_face_entry_differs_from_the_plain_zs_entry_next_to_a_face():
    faces, plain = BY_NAME["tx2-zs-faces-free6-bs2-4x12x1024"], BY_NAME["tx2-zs-bs2-4x12x1024"]
    assert faces.body().sizes == plain.body().sizes and faces.tau(faces.body()) == plain.tau(plain.body())
    a = oracle_steps(faces, states.uniform, n=1)
    pb = plain.body()
    b = pb.inner_view(oracle_steps(plain, states.uniform, n=1, body=pb).reshape(pb.pde.shape))
    d = differing(a, b)
    assert len(d) > 0
    sizes, bs = np.array(pb.sizes), pb.bs
    # one step: a face reaches bs nodes inward on its own axis, and no further
    assert ((d < bs) | (d >= sizes - bs)).any(axis=-1).all()
    for axis in range(3):
        assert (d[:, axis] == 0).any() and (d[:, axis] == sizes[axis] - 1).any(), axis


# ---- the part cut of rows longer than 512 -------------------------------------

ZCUT_PLACEMENTS = {"z509": 509, "z511": 511, "z512": 512, "z514": 514}


@pytest.mark.parametrize("Z", [64, 128, 512, 513, 1024])
def test_part_cut_placements_exist_exactly_beyond_512(Z):
    b, _ = body_of("iso", [4, 6, Z])
    nodes = states.impulse_nodes(b)
    assert set(ZCUT_PLACEMENTS) & set(nodes) == (set(ZCUT_PLACEMENTS) if Z > 512 else set())
    if Z > 512:
        for k, z in ZCUT_PLACEMENTS.items():
            assert nodes[k] == (2, 3, z)
    else:
        with pytest.raises(AssertionError):
            states.steps_zcut(b)
    b2, _ = body_of("iso2d", [9, 1024])
    assert not set(ZCUT_PLACEMENTS) & set(states.impulse_nodes(b2))


def test_steps_zcut_jumps_on_the_part_cut_in_every_component():
    b, _ = body_of("iso", [4, 6, 1024])
    states.steps_zcut(b)
    v = b.inner_view()
    assert (v[:, :, 511, :] != v[:, :, 512, :]).all()
    for z0, z1 in ((0, 512), (512, 1024)):  # constant on either side: ties and exact-zero differences
        assert (v[:, :, z0:z1, :] == v[:, :, z0:z0 + 1, :]).all()
    states.steps(b)
    assert (b.inner_view()[:, :, 511, :] == b.inner_view()[:, :, 512, :]).all()  # `steps` cuts at the wave seam
