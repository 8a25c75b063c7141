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
    may reach on the GPU (tests/test_gpu_nonfinite.py)."""
import numpy as np
import pytest

from tests import states
from tests.launch_catalog import MATERIAL_SETS

SIZES = {3: ([6, 7, 16], [9, 9, 16]), 2: ([9, 16], [12, 21])}
CASES = [(name, tuple(sizes)) for name in sorted(MATERIAL_SETS)
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
