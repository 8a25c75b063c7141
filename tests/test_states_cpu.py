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
from tests.launch_catalog import BY_NAME, MAP_64, MAP_1024, MATERIAL_SETS, partial_body

SIZES = {3: ([6, 7, 16], [9, 9, 16]), 2: ([9, 16], [12, 21])}
# the acoustic set last: the cases before it keep their ids
CASES = [(name, tuple(sizes)) for name in sorted(MATERIAL_SETS, key=lambda n: (n == "acoustic", n))
         for sizes in SIZES[2 if name.endswith("2d") else 3]]
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


@pytest.mark.parametrize("name", ["iso", "iso_het", "ortho", "ortho_het"])
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


# ---- the catalogue's ODE, face and face-map entries, on the oracle alone ------

FEATURE_ENTRIES = ("tx2-faces-ode-bs2-4x8x64", "tx2-zs-faces-free6-bs2-4x12x1024", "tx2-map-bs2-6x12x64")


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
                 "tx2-zs-ode-bs2-4x12x1024"):
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
    for name, conds in (("tx2-map-bs2-6x12x64", MAP_64), ("tx2-map-zs-bs2-4x10x1024", MAP_1024)):
        entry = BY_NAME[name]
        b0 = entry.body()
        got = oracle_steps(entry, states.uniform)
        everywhere = ("box", (-1e6,) * 3, (1e6,) * 3)  # partial_body cuts it to the condition's face
        whole = partial_body(b0.bs, b0.sizes, [(a, s, everywhere, v) for a, s, _, v in conds])
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
