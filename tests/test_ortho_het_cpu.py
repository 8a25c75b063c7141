"""The cross-ply helper (gcm_amd.host.cross_ply, no GPU): the 90-degree-about-z
permutation of the nine orthotropic constants, against the hand permutation
and the numpy restatement of the matrices in tests/test_ortho_cpu.py."""
import numpy as np
import pytest

from tests.test_ortho_cpu import MAT_A, MAT_B, ortho_matrices, ortho_tables, same_bits


@pytest.fixture(scope="module")
def host():
    import gcm_amd.host as host
    host.lib()
    return host


def hand_permutation(c):
    """x <-> y: c11 <-> c22, c13 <-> c23, c44 <-> c55; c12, c33, c66 stay."""
    c11, c12, c13, c22, c23, c33, c44, c55, c66 = c
    return (c22, c12, c23, c11, c13, c33, c55, c44, c66)


def test_cross_ply_equals_the_hand_permutation():
    from gcm_amd.host import cross_ply
    assert cross_ply(MAT_A[1]) == (180.0, 70.0, 50.0, 360.0, 60.0, 90.0, 20.0, 10.0, 30.0)
    for _, c in (MAT_A, MAT_B):
        p = cross_ply(c)
        assert p == hand_permutation(c)
        assert cross_ply(p) == tuple(c)  # a quarter turn twice: the same medium
        assert cross_ply(np.array(c)) == p and cross_ply(list(c)) == p
    with pytest.raises(ValueError):
        cross_ply([1.0] * 8)


def test_cross_ply_swaps_the_x_and_y_speeds():
    """The turned ply's x-axis speeds are the original's y-axis speeds (and the
    reverse) pair by pair; the z axis keeps its speeds with the shear pairs swapped."""
    from gcm_amd.host import cross_ply
    for rho, c in (MAT_A, MAT_B):
        L = ortho_tables(rho, c)[2]
        Lp = ortho_tables(rho, cross_ply(c))[2]
        assert same_bits(Lp[0], L[1]) and same_bits(Lp[1], L[0])
        assert same_bits(Lp[2], L[2][[2, 3, 0, 1, 4, 5, 6, 7, 8]])


def test_host_matrices_of_the_cross_ply_equal_the_restatement_bitwise(host):
    for rho, c in (MAT_A, MAT_B):
        p = host.cross_ply(c)
        U, U1, L = host.orthotropic_elastic_matrices(rho, p)
        _, wU, wU1, wL = ortho_matrices(rho, p)
        assert same_bits(U, wU) and same_bits(U1, wU1) and same_bits(L, wL), (rho, p)
