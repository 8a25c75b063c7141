"""Python access to the C++ host mirror (gcm_amd/host, lib/libgcm_host.so)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libgcm_host.so")
_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError(f"{HOST_LIB_PATH} not built: run __graft_entry__.build()")
        L = ctypes.CDLL(HOST_LIB_PATH)
        dp = ctypes.POINTER(ctypes.c_double)
        L.gcm_host_isotropic_elastic_matrices.argtypes = [ctypes.c_int, ctypes.c_double,
                                                          ctypes.c_double, ctypes.c_double,
                                                          dp, dp, dp]
        L.gcm_host_orthotropic_elastic_matrices.argtypes = [ctypes.c_double, dp, dp, dp, dp]
        L.gcm_host_orthotropic_from_isotropic.argtypes = [ctypes.c_double, ctypes.c_double,
                                                          ctypes.c_double, dp]
        L.gcm_host_orthotropic_from_isotropic.restype = None
        L.gcm_host_acoustic_matrices.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                 ctypes.c_double, dp, dp, dp]
        _lib = L
    return _lib


def isotropic_elastic_matrices(D: int, rho: float, lam: float, mu: float):
    """ElasticModel<D>::constructGcmMatrices (identity basis): U, U1 [D,M,M], L [D,M]."""
    M = D + D * (D + 1) // 2
    U = np.zeros((D, M, M)); U1 = np.zeros((D, M, M)); L = np.zeros((D, M))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if lib().gcm_host_isotropic_elastic_matrices(D, rho, lam, mu, dp(U), dp(U1), dp(L)) != 0:
        raise ValueError("bad isotropic material (needs rho > 0, mu > 0)")
    return U, U1, L


def orthotropic_elastic_matrices(rho: float, c):
    """ElasticModel<3>::constructGcmMatrices for an unrotated OrthotropicMaterial
    (c = c11, c12, c13, c22, c23, c33, c44, c55, c66): U, U1 [3,9,9], L [3,9]."""
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    if c.shape[0] != 9:
        raise ValueError("c must hold the nine elastic constants")
    U = np.zeros((3, 9, 9)); U1 = np.zeros((3, 9, 9)); L = np.zeros((3, 9))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if lib().gcm_host_orthotropic_elastic_matrices(rho, dp(c), dp(U), dp(U1), dp(L)) != 0:
        raise ValueError("bad orthotropic material (needs rho > 0 and positive diagonal constants)")
    return U, U1, L


def acoustic_matrices(D: int, rho: float, lam: float, mu: float = 0.0):
    """AcousticModel<D>::constructGcmMatrices (identity basis; mu is unused):
    U, U1 [D,M,M], L [D,M] with M = D + 1 (velocity, then pressure)."""
    M = D + 1
    U = np.zeros((D, M, M)); U1 = np.zeros((D, M, M)); L = np.zeros((D, M))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if lib().gcm_host_acoustic_matrices(D, rho, lam, mu, dp(U), dp(U1), dp(L)) != 0:
        raise ValueError("bad acoustic material (needs rho > 0, lambda > 0)")
    return U, U1, L


def cross_ply(c):
    """The nine constants (c11, c12, c13, c22, c23, c33, c44, c55, c66) of the same
    material turned by 90 degrees about z, i.e. the other ply of a 0/90 laminate:
    x and y change places, so c11 <-> c22, c13 <-> c23 and c44 <-> c55 swap while
    c12, c33 and c66 stay.  The result is again an unrotated orthotropic medium."""
    c = [float(v) for v in np.asarray(c, dtype=np.float64).reshape(-1)]
    if len(c) != 9:
        raise ValueError("c must hold the nine elastic constants")
    c11, c12, c13, c22, c23, c33, c44, c55, c66 = c
    return (c22, c12, c23, c11, c13, c33, c55, c44, c66)


def orthotropic_from_isotropic(rho: float, lam: float, mu: float) -> np.ndarray:
    """OrthotropicMaterial(IsotropicMaterial): c11, c12, c13, c22, c23, c33, c44, c55, c66."""
    c = np.zeros(9)
    lib().gcm_host_orthotropic_from_isotropic(rho, lam, mu, c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return c
