"""Unrotated orthotropic elastic media on the host (no GPU): OrthotropicMaterial,
ElasticModel<3>::constructGcmMatrices for it, the orthotropic wave map of the
set-up, and the additive ABI query.

The checker's matrices are restated here in numpy / Python floats, expression
by expression as ElasticModel<3>::constructNotRotated writes them
(ElasticModel3D.cpp:286-429); nothing below takes them from the product."""
import math

import numpy as np
import pytest

# the reference task's material (launcher/main.cpp:376-419) and one with nine distinct speeds
MAT_A = (4.0, (360.0, 70.0, 60.0, 180.0, 50.0, 90.0, 10.0, 20.0, 30.0))
MAT_B = (4.0, (360.0, 70.0, 70.0, 180.0, 70.0, 90.0, 10.0, 10.0, 10.0))
EQUALITY_TOLERANCE = 1e-9  # util/math/GridCharacteristicMethod.hpp:60-69


def ortho_matrices(rho, c):
    """A, U, U1 [3, 9, 9] and L [3, 9] of the unrotated orthotropic material, IEEE
    double operations in the reference's order."""
    c11, c12, c13, c22, c23, c33, c44, c55, c66 = (float(v) for v in c)
    rho = float(rho)
    sqrt = math.sqrt
    Z = 0.0
    A = np.zeros((3, 9, 9)); U = np.zeros((3, 9, 9)); U1 = np.zeros((3, 9, 9)); L = np.zeros((3, 9))

    A[0, 0, 3] = A[0, 1, 4] = A[0, 2, 5] = -1.0 / rho
    A[0, 3, 0] = -c11; A[0, 4, 1] = -c66; A[0, 5, 2] = -c55; A[0, 6, 0] = -c12; A[0, 8, 0] = -c13
    L[0] = [-sqrt(c66 / rho), sqrt(c66 / rho), -sqrt(c55 / rho), sqrt(c55 / rho),
            -sqrt(c11 / rho), sqrt(c11 / rho), Z, Z, Z]
    U[0] = [
        [0, 1.0, 0, 0, 1.0 / (sqrt(c66) * sqrt(rho)), 0, 0, 0, 0],
        [0, 1.0, 0, 0, -1.0 / (sqrt(c66) * sqrt(rho)), 0, 0, 0, 0],
        [0, 0, 1.0, 0, 0, 1.0 / (sqrt(c55) * sqrt(rho)), 0, 0, 0],
        [0, 0, 1.0, 0, 0, -1.0 / (sqrt(c55) * sqrt(rho)), 0, 0, 0],
        [1.0, 0, 0, 1.0 / (sqrt(c11) * sqrt(rho)), 0, 0, 0, 0, 0],
        [1.0, 0, 0, -1.0 / (sqrt(c11) * sqrt(rho)), 0, 0, 0, 0, 0],
        [0, 0, 0, -c12 / c11, 0, 0, 1.0, 0, 0.0],
        [0, 0, 0, 0, 0, 0, 0, 1.0, 0],
        [0, 0, 0, -(1.0 * c13) / c11, 0, 0, 0, 0, 1.0]]
    U1[0] = [
        [0, 0, 0, 0, 0.5, 0.5, 0, 0, 0],
        [0.5, 0.5, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0.5, 0.5, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0.5 * sqrt(c11) * sqrt(rho), -0.5 * sqrt(c11) * sqrt(rho), 0, 0, 0],
        [0.5 * sqrt(c66) * sqrt(rho), -0.5 * sqrt(c66) * sqrt(rho), 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0.5 * sqrt(c55) * sqrt(rho), -0.5 * sqrt(c55) * sqrt(rho), 0, 0, 0, 0, 0],
        [0, 0, 0, 0, (0.5 * c12 * sqrt(rho)) / sqrt(c11), -(0.5 * c12 * sqrt(rho)) / sqrt(c11), 1, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 1, 0],
        [0, 0, 0, 0, (0.5 * c13 * sqrt(rho)) / sqrt(c11), -(0.5 * c13 * sqrt(rho)) / sqrt(c11), 0, 0, 1]]

    A[1, 0, 4] = A[1, 1, 6] = A[1, 2, 7] = -1.0 / rho
    A[1, 3, 1] = -c12; A[1, 4, 0] = -c66; A[1, 6, 1] = -c22; A[1, 7, 2] = -c44; A[1, 8, 1] = -c23
    L[1] = [-sqrt(c66 / rho), sqrt(c66 / rho), -sqrt(c44 / rho), sqrt(c44 / rho),
            -sqrt(c22 / rho), sqrt(c22 / rho), Z, Z, Z]
    U[1] = [
        [1.0, 0, 0, 0, 1.0 / (sqrt(c66) * sqrt(rho)), 0, 0, 0, 0],
        [1.0, 0, 0, 0, -1.0 / (sqrt(c66) * sqrt(rho)), 0, 0, 0, 0],
        [0, 0, 1.0, 0, 0, 0, 0, 1.0 / (sqrt(c44) * sqrt(rho)), 0],
        [0, 0, 1.0, 0, 0, 0, 0, -1.0 / (sqrt(c44) * sqrt(rho)), 0],
        [0, 1.0, 0, 0, 0, 0, 1.0 / (sqrt(c22) * sqrt(rho)), 0, 0],
        [0, 1.0, 0, 0, 0, 0, -1.0 / (sqrt(c22) * sqrt(rho)), 0, 0],
        [0, 0, 0, 1.0, 0, 0, -c12 / c22, 0, 0.0],
        [0, 0, 0, 0, 0, 1.0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, -(1.0 * c23) / c22, 0, 1.0]]
    U1[1] = [
        [0.5, 0.5, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0.5, 0.5, 0, 0, 0],
        [0, 0, 0.5, 0.5, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, (0.5 * c12) / sqrt(c22 / rho), -(0.5 * c12) / sqrt(c22 / rho), 1, 0, 0],
        [0.5 * sqrt(c66) * sqrt(rho), -0.5 * sqrt(c66) * sqrt(rho), 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 1, 0],
        [0, 0, 0, 0, 0.5 * sqrt(c22) * sqrt(rho), -0.5 * sqrt(c22) * sqrt(rho), 0, 0, 0],
        [0, 0, 0.5 * sqrt(c44) * sqrt(rho), -0.5 * sqrt(c44) * sqrt(rho), 0, 0, 0, 0, 0],
        [0, 0, 0, 0, (0.5 * c23 * sqrt(rho)) / sqrt(c22), -(0.5 * c23 * sqrt(rho)) / sqrt(c22), 0, 0, 1]]

    A[2, 0, 5] = A[2, 1, 7] = A[2, 2, 8] = -1.0 / rho
    A[2, 3, 2] = -c13; A[2, 5, 0] = -c55; A[2, 6, 2] = -c23; A[2, 7, 1] = -c44; A[2, 8, 2] = -c33
    L[2] = [-sqrt(c55 / rho), sqrt(c55 / rho), -sqrt(c44 / rho), sqrt(c44 / rho),
            -sqrt(c33 / rho), sqrt(c33 / rho), Z, Z, Z]
    U[2] = [
        [1.0, 0, 0, 0, 0, 1.0 / (sqrt(c55) * sqrt(rho)), 0, 0, 0],
        [1.0, 0, 0, 0, 0, -1.0 / (sqrt(c55) * sqrt(rho)), 0, 0, 0],
        [0, 1.0, 0, 0, 0, 0, 0, 1.0 / (sqrt(c44) * sqrt(rho)), 0],
        [0, 1.0, 0, 0, 0, 0, 0, -1.0 / (sqrt(c44) * sqrt(rho)), 0],
        [0, 0, 1.0, 0, 0, 0, 0, 0, 1.0 / (sqrt(c33) * sqrt(rho))],
        [0, 0, 1.0, 0, 0, 0, 0, 0, -1.0 / (sqrt(c33) * sqrt(rho))],
        [0, 0, 0, 1.0, 0, 0, 0, 0, -(1.0 * c13) / c33],
        [0, 0, 0, 0, 1.0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 1.0, 0, -(1.0 * c23) / c33]]
    U1[2] = [
        [0.5, 0.5, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0.5, 0.5, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0.5, 0.5, 0, 0, 0],
        [0, 0, 0, 0, (0.5 * c13 * sqrt(rho)) / sqrt(c33), -(0.5 * c13 * sqrt(rho)) / sqrt(c33), 1, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 1, 0],
        [0.5 * sqrt(c55) * sqrt(rho), -0.5 * sqrt(c55) * sqrt(rho), 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, (0.5 * c23 * sqrt(rho)) / sqrt(c33), -(0.5 * c23 * sqrt(rho)) / sqrt(c33), 0, 0, 1],
        [0, 0, 0.5 * sqrt(c44) * sqrt(rho), -0.5 * sqrt(c44) * sqrt(rho), 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0.5 * sqrt(c33) * sqrt(rho), -0.5 * sqrt(c33) * sqrt(rho), 0, 0, 0]]
    return A, U, U1, L


def ortho_tables(rho, c):
    """(U, U1, L) as oracle.Body.tables holds them."""
    _, U, U1, L = ortho_matrices(rho, c)
    return U, U1, L


def max_eigenvalue(L):
    """GcmMatrices::getMaximalEigenvalue (GridCharacteristicMethod.hpp:46-61)."""
    ans = 0.0
    for s in range(3):
        for k in range(9):
            ans = max(ans, abs(float(L[s, k])))
    return ans


def random_materials(n=200, seed=20260311):
    """OrthotropicMaterial::generateRandomMaterial (OrthotropicMaterial.cpp:35-59):
    H^T H of a uniform [1, 1e3] 3x3 matrix, shear constants in [1, 1e6], rho in [0.01, 100]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rho = float(rng.uniform(0.01, 100.0))
        H = rng.uniform(1.0, 1e3, (3, 3))
        S = H.T @ H
        sh = rng.uniform(1.0, 1e6, 3)
        out.append((rho, (float(S[0, 0]), float(S[0, 1]), float(S[0, 2]), float(S[1, 1]), float(S[1, 2]),
                          float(S[2, 2]), float(sh[0]), float(sh[1]), float(sh[2]))))
    return out


MATERIALS = [MAT_A, MAT_B] + random_materials()


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def host():
    import gcm_amd.host as host
    host.lib()
    return host


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def test_host_matrices_equal_the_restatement_bitwise(host):
    """array_equal, signbits included, for A, B and 200 random materials."""
    for rho, c in MATERIALS:
        U, U1, L = host.orthotropic_elastic_matrices(rho, c)
        _, wU, wU1, wL = ortho_matrices(rho, c)
        assert np.array_equal(U, wU) and np.array_equal(U1, wU1) and np.array_equal(L, wL), (rho, c)
        assert same_bits(U, wU) and same_bits(U1, wU1) and same_bits(L, wL), (rho, c)


def near(P, Q, eps):
    """TestGcmMatrices.cpp:19-25 with `relative`: per entry, eps * (|p| + |q|) where
    that scale exceeds eps, else eps."""
    scale = np.abs(P) + np.abs(Q)
    bound = np.where(scale > eps, eps * scale, eps)
    return bool(np.all(np.abs(P - Q) <= bound))


def test_decomposition_and_sparsity(host):
    """checkDecomposition (GridCharacteristicMethod.hpp:60-69): traces within
    EQUALITY_TOLERANCE, the three products within 1000 x that; nnz(U) = 17,
    nnz(U1) = 19 on every axis."""
    eps = EQUALITY_TOLERANCE
    for rho, c in MATERIALS:
        U, U1, L = host.orthotropic_elastic_matrices(rho, c)
        A = ortho_matrices(rho, c)[0]
        for s in range(3):
            Ld = np.diag(L[s])
            assert abs(np.trace(A[s]) - np.trace(Ld)) <= eps
            assert near(A[s] @ U1[s], U1[s] @ Ld, eps * 1000), (rho, c, s)
            assert near(U[s] @ A[s], Ld @ U[s], eps * 1000), (rho, c, s)
            assert near(U[s] @ U1[s], np.eye(9), eps * 1000), (rho, c, s)
            assert np.count_nonzero(U[s]) == 17 and np.count_nonzero(U1[s]) == 19


def test_bad_materials_are_refused(host):
    rho, c = MAT_A
    with pytest.raises(ValueError):
        host.orthotropic_elastic_matrices(0.0, c)
    for i in (0, 3, 5, 6, 7, 8):  # the six diagonal constants
        bad = list(c)
        bad[i] = 0.0
        with pytest.raises(ValueError):
            host.orthotropic_elastic_matrices(rho, bad)


def test_converting_constructor_from_isotropic(host):
    """OrthotropicMaterial(IsotropicMaterial) (OrthotropicMaterial.cpp:7-18)."""
    lam, mu = 2.0, 0.75
    c = host.orthotropic_from_isotropic(4.0, lam, mu)
    c11, c12, c13, c22, c23, c33, c44, c55, c66 = c.tolist()
    assert c11 == c22 == c33 == lam + 2 * mu
    assert c44 == c55 == c66 == mu
    assert c12 == c13 == c23 == lam


def ortho_task(H, D=3, angles=(0.0, 0.0, 0.0), sizes=(6, 5, 4)):
    t = H.Task()
    t.dimensionality = D
    t.border_size = 2
    t.h = [0.5, 0.4, 0.3][:D]
    t.courant = 0.9
    t.number_of_snaps = 1
    t.add_body(0, list(sizes[:D]), [0] * D)
    t.set_default_orthotropic_material(MAT_A[0], list(MAT_A[1]), angles=list(angles))
    return t


def test_rotated_and_lower_dimensional_media_raise(H):
    """Non-zero angles, D = 2 and D = 1 throw gcm::Exception."""
    with pytest.raises(H.GcmException):
        H.host_state(ortho_task(H, angles=(0.0, 0.3, 0.0)), 0)
    with pytest.raises(H.GcmException):
        H.host_state(ortho_task(H, D=2), 0)
    with pytest.raises(H.GcmException):
        H.host_state(ortho_task(H, D=1), 0)
    with pytest.raises(H.GcmException):
        H.Task().set_default_orthotropic_material(4.0, [1.0] * 8)


def test_setup_with_orthotropic_waves(H):
    """The GPU-free set-up with an orthotropic default material: an initial wave is
    U1[direction][:, column] * (value / current) with the orthotropic columns
    (Model.cpp:42-49): P_FORWARD 5, S2_BACKWARD 2."""
    _, U1, L = ortho_tables(*MAT_A)
    for wave, col, quantity, comp in (("P_FORWARD", 5, "Vy", 1), ("S2_BACKWARD", 2, "Vz", 2)):
        t = ortho_task(H)
        t.add_initial_wave(("infinite",), wave, 1, quantity, 2.5)
        st = H.host_state(t, 0)
        v = U1[1][:, col].copy()
        want = v * (2.5 / float(v[comp]))
        got = st["pde"][2:-2, 2:-2, 2:-2].reshape(-1, 9)
        assert np.array_equal(got, np.broadcast_to(want, got.shape)), wave
        assert st["maximal_eigenvalue"] == max_eigenvalue(L)
    # an isotropic area inside an orthotropic body is converted (c11 = lam + 2 mu, ...)
    t = ortho_task(H)
    t.add_material(("infinite",), 4.0, 2.0, 1.0)
    st = H.host_state(t, 0)
    assert st["n_conditions"] == 2
    assert st["maximal_eigenvalue"] == max(max_eigenvalue(L), math.sqrt((2.0 + 2 * 1.0) / 4.0))


def test_isotropic_setup_keeps_its_wave_columns(H):
    """The isotropic calls keep their signatures and columns (P_FORWARD 0)."""
    from oracle import oracle as O
    t = H.Task()
    t.dimensionality = 3
    t.border_size = 2
    t.h = [1.0, 1.0, 1.0]
    t.courant = 0.9
    t.number_of_snaps = 1
    t.add_body(0, [4, 4, 4], [0, 0, 0])
    t.set_default_material(4.0, 2.0, 1.0)
    t.add_initial_wave(("infinite",), "P_FORWARD", 0, "Vx", 1.0)
    st = H.host_state(t, 0)
    _, U1, _ = O.isotropic_elastic_matrices(3, 4.0, 2.0, 1.0)
    v = U1[0][:, 0]
    got = st["pde"][2:-2, 2:-2, 2:-2].reshape(-1, 9)
    assert np.array_equal(got, np.broadcast_to(v * (1.0 / float(v[0])), got.shape))


def test_library_exports_the_structure_query():
    import gcm_amd
    from gcm_amd.gcmx import SYMBOLS
    assert hasattr(gcm_amd.lib(), "gcmx_matrix_structure")
    assert "gcmx_matrix_structure" in SYMBOLS
    assert gcm_amd.lib().gcmx_abi_version() == 3
