"""The one-plane kernel (plane_step.hpp) is one template compiled into four
objects: kernels_xyz.hip and kernels_ortho.hip, each as the exact and as the FMA
build.  Were its instances to share a symbol between two objects, the linker
would keep one body for both gcmx_set_fp_mode settings without a word.  So for
each launch below, two steps at Courant 0.9 on a non-dyadic material (its
products and sums round, so a contracted multiply-add shows):
  * the exact build equals the oracle's stage sequence bitwise,
  * the FMA build differs from the exact build in at least one bit,
  * the FMA build stays within 1e-10 relative L2 of the oracle, the bound of
    tests/test_gpu_fma.py and tests/test_gpu_ortho.py.
The orthotropic tables are the numpy restatement of tests/test_ortho_cpu.py."""
import numpy as np
import pytest

from tests.helpers import context_for, oracle_body, random_materials, random_state
from tests.test_ortho_cpu import max_eigenvalue, ortho_tables

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_fma.py: TOL; tests/test_gpu_ortho.py: test_fma_build_within_tolerance
ISO = (1.3, 2.7, 0.9)  # rho, lambda, mu
# rho, (c11, c12, c13, c22, c23, c33, c44, c55, c66): three unequal stiffness rows
ORTHO_A = (1.3, (36.7, 7.3, 6.1, 18.9, 5.3, 9.7, 1.1, 2.3, 3.7))
ORTHO_B = (1.7, (29.3, 6.7, 5.9, 21.1, 4.3, 11.3, 1.9, 2.9, 3.1))
H_ORTHO = (0.5, 0.4, 0.3)


def iso_body():
    """The isotropic one-plane path: borderSize 3 (k_step_tx2 takes 1 and 2)."""
    b = oracle_body(3, 3, [4, 7, 100], materials=(ISO,))
    return b, "k_fused_xyz<3, 128, KF0, !UNI{}>"


def ortho_body(mats):
    b = oracle_body(3, 2, [6, 9, 37], h=H_ORTHO, materials=((4.0, 2.0, 1.0),) * len(mats))
    b.tables = [ortho_tables(*m) for m in mats]
    b.maximal_eigenvalue = max(max_eigenvalue(t[2]) for t in b.tables)
    if len(mats) > 1:
        random_materials(b, seed=5)
    return b, "k_step_ortho<2, 64, KF0{}{{}}>".format(", HET" if len(mats) > 1 else "")


CASES = {"iso": iso_body, "ortho": lambda: ortho_body((ORTHO_A,)), "ortho_het": lambda: ortho_body((ORTHO_A, ORTHO_B))}


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_and_fma_builds_are_two_kernels(case):
    import gcm_amd as G
    G.lib()
    b, kernel = CASES[case]()
    random_state(b, seed=31, ghosts=False)
    tau = 0.9 * min(b.h[:3]) / b.maximal_eigenvalue
    ex, fm = context_for(b), context_for(b)
    fm.fp_mode = G.FP_FMA
    assert ex.fp_mode == G.FP_EXACT and fm.fp_mode == G.FP_FMA
    for c in (ex, fm):
        c.profile(True)
    for _ in range(2):
        for s in range(3):
            b.stage(s, tau)
        ex.step(tau)
        fm.step(tau)
    names = lambda c: [v["kernel"] for v in c.profile_read().values() if v["launches"] > 0]
    assert names(ex) == [kernel.format("")], names(ex)
    assert names(fm) == [kernel.format(", FMA")], names(fm)
    want, exact, fma = b.pde, ex.download(), fm.download()
    ex.close(); fm.close()
    nbits = int(np.count_nonzero(exact != fma))
    rel = float(np.linalg.norm(fma - want) / np.linalg.norm(want))
    print(f"{case}: exact == oracle: {np.array_equal(exact, want)}; values where FMA != exact: {nbits} of "
          f"{exact.size}; FMA vs oracle relative L2 {rel:.3e}")
    assert np.array_equal(exact, want), f"{int(np.count_nonzero(exact != want))} values of the exact build differ"
    assert nbits > 0, "the FMA build gave the exact build's bits: one kernel body behind both builds?"
    assert rel <= TOL, rel
