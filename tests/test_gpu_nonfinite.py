"""Non-finite input: where a NaN or an Inf may go.

The random state with one inner node tainted (the centre; for rows of 128 and
more also the node at z = 63, next to the wave seam; for rows longer than 512
also the node at z = 511, next to the part cut), one step, exact build.
R is the set of nodes where the oracle's result has a non-finite component.

  1. Outside R the GPU result is finite and equals the oracle bit for bit.  The
     kernels skip structural-zero matrix terms where the oracle forms 0 * NaN,
     so they read a subset of what the oracle reads: outside R no tainted value
     is read, whatever the limiter does with it.  A taint that leaves R came
     through a wrong lane, row-ring slot or seam.
  2. Inside R the values are unspecified (v_min_f64 / v_max_f64 return the
     operand that is not NaN; skipped terms never see the taint); how many nodes
     of R are non-finite on the GPU is printed per case and tabulated in
     DESIGN.md §3.5.
  3. The one-pass kernel and the generic stages need not agree inside R.

tests/test_states_cpu.py asserts the oracle fact this rests on: R is the
(2 bs + 1)^3 box around the tainted node, clipped to the grid, all components
(the acoustic medium's R is stated there too)."""
import numpy as np
import pytest

from tests import states
from tests.launch_catalog import CATALOG

pytestmark = pytest.mark.gpu

VARIANTS = ("vx-nan", "s-nan", "vx-inf")
# the slab group and the split stages add no kernel of their own here
ENTRIES = [e for e in CATALOG if e.kind != "slabs" and not e.name.startswith("split-")]


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def taint_nodes(body):
    nodes = states.impulse_nodes(body)
    return [nodes[k] for k in ("centre", "z63", "z511") if k in nodes]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("entry", ENTRIES, ids=repr)
def test_taint_stays_inside_the_oracles_region(G, entry, variant):
    for node in taint_nodes(entry.body()):
        body = entry.body()
        states.taint(body, node, variant)
        run = entry.start(body, G.FP_EXACT)
        got = run.step(0.0)[-1]
        run.check_kernels()
        run.close()
        want = entry.oracle_step(body, 0.0)[-1]
        R = (~np.isfinite(want)).any(axis=-1)
        assert R[entry.node_of(body, node)], "the oracle keeps the tainted node tainted"
        what = f"{entry.name} {variant} at {node}"
        out = ~R
        assert np.isfinite(got[out]).all(), \
            f"{what}: {int((~np.isfinite(got[out])).any(axis=-1).sum())} nodes outside R are non-finite"
        a, b = got[out].view(np.uint64), want[out].view(np.uint64)
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} values outside R differ from the oracle"
        bad = (~np.isfinite(got)).any(axis=-1) & R
        print(f"NONFINITE {entry.name} {variant} z={node[-1]}: R {int(R.sum())} nodes, "
              f"GPU non-finite in {int(bad.sum())}")
