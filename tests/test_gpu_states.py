"""Every catalogue launch (tests/launch_catalog.py) on the structured states of
tests/states.py: a lone impulse (at the centre, in the first and the last inner
node, on both sides of the wave seam of long rows, and for rows longer than 512
on both sides of the part cut and in the columns next to those the seam kernel
stores), piecewise-constant blocks (for rows longer than 512 also with the jump
on the part cut), a linear ramp, and the random state scaled by 2^-1000, 2^1000
and 2^-1060.  Two steps each.

Exact build: no non-finite value on either side, and equal to the oracle with
+0 and -0 identified: (got + 0.0) and (want + 0.0) have the
same bits.  The count of zeros whose sign differs is printed, for information.

FMA build: within 1e-10 relative L2 of the exact build (the suite's bound; no
ratio where the exact norm is 0).  The scaled states give the contracted kernels
an exact check of their own: scaling by a power of two commutes with every
rounding of a fused multiply-add while nothing overflows or underflows, so the
result from scaled(+-1000) must be ldexp of the same build's unscaled result,
bit for bit, with no oracle involved (a value that 2^-1000 takes below the
normal range -- the contracted residual of a sum that cancels exactly -- is held
to a few subnormal spacings).  scaled(-1060) lives among the subnormals,
where that no longer holds: finite, and in the exact build equal to the oracle."""
import numpy as np
import pytest

from tests import states
from tests.launch_catalog import CATALOG

pytestmark = pytest.mark.gpu

STEPS = 2
TOL = 1e-10
TINY = float(np.finfo(np.float64).tiny)
SUBNORMAL_SLACK = float(np.ldexp(1.0, -1074 + 12))  # test_scaled_states: where the scaled result underflows
PLACEMENTS = ("centre", "first", "last", "z63", "z64", "z509", "z511", "z512", "z514")
FAMILIES = tuple(f"impulse-{p}" for p in PLACEMENTS) + ("steps", "steps-zcut", "ramp")


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def fill(body, family):
    if family.startswith("impulse-"):
        return states.impulse(body, family[len("impulse-"):])
    {"steps": states.steps, "steps-zcut": states.steps_zcut, "ramp": states.ramp,
     "uniform": states.uniform}[family](body)


# rows shorter than 128 have no wave seam, rows up to 512 no part cut: nothing
# to place there
_PLACED = {e.name: set(states.impulse_nodes(e.body())) for e in CATALOG}
_ZCUT = {e.name for e in CATALOG if e.body().D == 3 and e.body().sizes[2] > states.Z_PART}
CASES = [(e, f) for e in CATALOG for f in FAMILIES
         if (f[len("impulse-"):] in _PLACED[e.name] if f.startswith("impulse-")
             else f != "steps-zcut" or e.name in _ZCUT)]


def run_oracle(entry, fill_body):
    body = entry.body()
    fill_body(body)
    out, t = [], 0.0
    for _ in range(STEPS):
        out += entry.oracle_step(body, t)
        t += entry.tau(body)
    return out


def run_gpu(entry, fill_body, fp):
    body = entry.body()
    fill_body(body)
    run = entry.start(body, fp)
    out, t = [], 0.0
    for _ in range(STEPS):
        out += run.step(t)
        t += run.tau
    names = run.check_kernels()
    run.close()
    return out, names


def assert_canonical(got, want, what):
    assert np.isfinite(want).all(), f"{what}: the oracle has non-finite values"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite values"
    a, b = states.canonical_bits(got), states.canonical_bits(want)
    if not np.array_equal(a, b):
        diff = a != b
        i0 = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} values differ; first at {i0}: "
                             f"got {got[i0]!r} want {want[i0]!r}")
    return states.sign_differing_zeros(got, want)


def assert_fma_close(fma, exact, what):
    assert np.isfinite(fma).all(), f"{what}: {int((~np.isfinite(fma)).sum())} non-finite values"
    norm = float(np.linalg.norm(exact))
    if norm == 0.0 or not np.isfinite(norm):
        return 0.0
    r = float(np.linalg.norm(fma - exact)) / norm
    assert r <= TOL, f"{what}: FMA against exact, relative L2 {r:.3e} > {TOL}"
    return r


def assert_same_support(got, want, what):
    a, b = (got != 0.0).any(axis=-1), (want != 0.0).any(axis=-1)
    if not np.array_equal(a, b):
        stray = np.argwhere(a != b)[0]
        raise AssertionError(f"{what}: non-zero nodes differ from the oracle's; first stray node "
                             f"{tuple(int(v) for v in stray)} ({'GPU' if a[tuple(stray)] else 'oracle'} only)")


def assert_within_reach(got, node, radius, what):
    """The contracted build may leave a rounding residual where the exact sum
    cancels to zero, but only where the stencil reaches: a stage reads at most
    borderSize nodes either way, so after n steps nothing beyond n * borderSize
    nodes of the impulse, along any axis, may be non-zero."""
    hit = np.argwhere((got != 0.0).any(axis=-1))
    far = hit[(np.abs(hit - np.array(node)) > radius).any(axis=-1)]
    assert far.size == 0, f"{what}: non-zero node {tuple(int(v) for v in far[0])} is more than {radius} from {node}"


@pytest.mark.parametrize("entry,family", CASES, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_structured_state(G, entry, family):
    want = run_oracle(entry, lambda b: fill(b, family))
    node, bs = fill(entry.body(), family), entry.body().bs
    exact, _ = run_gpu(entry, lambda b: fill(b, family), G.FP_EXACT)
    fma, _ = run_gpu(entry, lambda b: fill(b, family), G.FP_FMA)
    signs, worst = 0, 0.0
    for k, (e, f, w) in enumerate(zip(exact, fma, want)):
        what = f"{entry.name} {family} state {k}"
        signs += assert_canonical(e, w, what)
        if family.startswith("impulse-"):
            assert_same_support(e, w, what)
            assert_within_reach(f, entry.node_of(entry.body(), node), bs * (1 + k // (len(want) // STEPS)),
                                what + " (FMA)")
        worst = max(worst, assert_fma_close(f, e, what))
    print(f"SIGNED-ZEROS {entry.name} {family}: {signs}")
    print(f"FMA-RATIO {entry.name} {family}: {worst:.3e}")


@pytest.mark.parametrize("entry", CATALOG, ids=repr)
def test_scaled_states(G, entry):
    want = {e: run_oracle(entry, lambda b: states.scaled(b, e)) for e in states.SCALES}
    base = {fp: run_gpu(entry, states.uniform, fp)[0] for fp in (G.FP_EXACT, G.FP_FMA)}
    signs, worst = 0, 0.0
    for e in states.SCALES:
        exact, _ = run_gpu(entry, lambda b: states.scaled(b, e), G.FP_EXACT)
        fma, _ = run_gpu(entry, lambda b: states.scaled(b, e), G.FP_FMA)
        for k, (x, f, w) in enumerate(zip(exact, fma, want[e])):
            what = f"{entry.name} scaled({e}) state {k}"
            signs += assert_canonical(x, w, what)
            assert np.isfinite(f).all(), f"{what}: FMA build, {int((~np.isfinite(f)).sum())} non-finite values"
            if e == -1060:
                continue
            worst = max(worst, assert_fma_close(np.ldexp(f, -e), np.ldexp(x, -e), what))  # norms taken near 1
            for name, got, fp in (("exact", x, G.FP_EXACT), ("FMA", f, G.FP_FMA)):
                ref = np.ldexp(base[fp][k], e)
                diff = got.view(np.uint64) != ref.view(np.uint64)
                # the identity's own condition: nothing underflows.  Where a sum cancels
                # exactly (a free surface's normal stress) the contracted build leaves a
                # residual of ~1e-17, which 2^-1000 takes among the subnormals: the scaled
                # run's roundings there are to multiples of 2^-1074, at most 2^-1075 off
                # each, in fewer than 2^9 operations per value over the three stages
                # (nine U1 terms of three U terms of an interpolant of <= 8 operations),
                # amplified by less than 2^3 on the way (|u|, |u1| <= 2.5, each sum a
                # stable scheme's).  So a subnormal value is held to 2^12 spacings, 2^-50
                # of the smallest normal number; every normal one and every zero bitwise.
                underflowed = (ref != 0.0) & (np.abs(ref) < TINY)
                diff &= ~(underflowed & (np.abs(got - ref) <= SUBNORMAL_SLACK))
                if diff.any():
                    i0 = tuple(int(v) for v in np.argwhere(diff)[0])
                    raise AssertionError(f"{what}: {name} build, {int(diff.sum())} values are not ldexp of the "
                                         f"unscaled result; first at {i0}: got {got[i0]!r} want {ref[i0]!r}")
                if underflowed.any():
                    print(f"UNDERFLOWED {entry.name} scaled({e}) state {k} {name}: {int(underflowed.sum())} values")
    print(f"SIGNED-ZEROS {entry.name} scaled: {signs}")
    print(f"FMA-RATIO {entry.name} scaled: {worst:.3e}")
