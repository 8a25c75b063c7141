"""Acoustic reference for the tests (helper, not collected): a numpy
restatement of AcousticModel<D>::constructGcmMatrix for the identity calculation
basis (rheology/models/AcousticModel.hpp:214-317), oracle bodies that hold
M = D + 1 components, the acoustic cubic border rule and a small engine loop
with the AbstractEngine clock semantics.  Nothing here comes from the product.

The PDE vector is Vx..V(D-1), then the pressure at index D
(rheology/variables/AcousticVariables.hpp).  The oracle's stage, random fill and
interpolators take M from the grid struct, so `Body.stage` runs unchanged."""
import ctypes
import math

import numpy as np

from oracle import oracle as O

EQUALITY_TOLERANCE = 1e-9  # util/infrastructure/Types.hpp:10 (real = double)


def local_basis(D, axis):
    """linal::createLocalBasis(e_axis) (linal/basis.hpp:49-65) with
    perpendicularClockwise (linal/geometry.hpp:35-52): columns (tau1, tau2, n),
    the reference's operations in the reference's order (signed zeros kept)."""
    n = np.zeros(3)
    n[axis] = 1.0
    B = np.zeros((D, D))
    if D == 1:
        B[0, 0] = n[0]
    elif D == 2:
        tau = (n[1], -n[0])
        B[0, 0], B[0, 1] = tau[0], n[0]
        B[1, 0], B[1, 1] = tau[1], n[1]
    else:
        ans = np.array([n[1], -n[0], 0.0])
        if n[0] == 0 and n[1] == 0:
            ans = np.array([n[2], 0.0, 0.0])
        lv = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        la = math.sqrt(ans[0] * ans[0] + ans[1] * ans[1] + ans[2] * ans[2])
        t1 = np.array([(ans[i] * lv) / la for i in range(3)])
        t2 = np.array([n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]])
        B[:, 0], B[:, 1], B[:, 2] = t1, t2, n
    return B


def acoustic_tables(D, rho, lam, with_A=False):
    """U, U1 [D, M, M] and L [D, M] of AcousticModel<D> for the identity basis;
    with_A: also A [D, M, M] as constructGcmMatrix assembles it (:226-234)."""
    M = D + 1
    U = np.zeros((D, M, M)); U1 = np.zeros((D, M, M)); L = np.zeros((D, M)); A = np.zeros((D, M, M))
    c1 = math.sqrt(lam / rho)
    l = 1.0
    alpha = 0.5
    for s in range(D):
        B = local_basis(D, s)
        nn = [B[:, (i + D - 1) % D].copy() for i in range(D)]  # n[0] = the normal, then the tangents
        n = B[:, D - 1]
        A[s, D, :D] = l * lam * n     # setRow(D, {velocity l lambda n, pressure 0})
        A[s, :D, D] = l / rho * n     # setColumn(D, {velocity l / rho n, pressure 0})
        A[s, D, D] = 0.0
        L[s, 0] = l * c1
        L[s, 1] = -l * c1
        U1[s, :D, 0] = nn[0]; U1[s, D, 0] = c1 * rho
        U1[s, :D, 1] = nn[0]; U1[s, D, 1] = -(c1 * rho)
        U[s, 0, :D] = alpha * nn[0]; U[s, 0, D] = alpha / (c1 * rho)
        U[s, 1, :D] = alpha * nn[0]; U[s, 1, D] = -(alpha / (c1 * rho))
        for i in range(1, D):
            U1[s, :D, i + 1] = nn[i]; U1[s, D, i + 1] = 0.0
            U[s, i + 1, :D] = nn[i]; U[s, i + 1, D] = 0.0
    return (U, U1, L, A) if with_A else (U, U1, L)


def max_eigenvalue(L):
    """getMaximalEigenvalue: fmax over fabs(L(i)), axes and components."""
    ans = 0.0
    for s in range(L.shape[0]):
        for k in range(L.shape[1]):
            ans = max(ans, abs(L[s, k]))
    return ans


def acoustic_body(D, bs, sizes, h=None, rho=2.0, lam=8.0, start=None, tables=None):
    """An oracle Body with zero state whose arrays and tables are acoustic:
    M = D + 1 in the body and in the grid struct the C stage reads."""
    h = list(h) if h is not None else [1.0] * D
    start = list(start) if start is not None else [0] * D
    t = O.Task(D=D, border_size=bs, h=h, cubics={0: (list(sizes), start)}, courant=1.0,
               default_material=O.Material(1.0, 1.0, 1.0), number_of_snaps=1)
    b = O.Engine(t).bodies[0]
    b.M = D + 1
    b.g = O._OgGrid(D, b.M, b.bs, (ctypes.c_int * 3)(*b.sizes), (ctypes.c_int * 3)(*b.start),
                    (ctypes.c_double * 3)(*b.h))
    b.pde = np.zeros((b.n_all, b.M))
    b.pde_new = np.zeros((b.n_all, b.M))
    b.tables = [tables if tables is not None else acoustic_tables(D, rho, lam)]
    b.maximal_eigenvalue = max_eigenvalue(b.tables[0][2])
    b.border = []
    return b


def step(b, tau):
    for s in range(b.D):
        b.stage(s, tau)


def quantity_index(D, q):
    """AcousticVariables::QUANTITIES: Vx.., and PRESSURE = component D."""
    if q in ("Vx", "Vy", "Vz"):
        i = "xyz".index(q[1])
        if i < D:
            return i
    if q == "PRESSURE":
        return D
    raise KeyError(q)


def face_nodes(b, axis, side, area=("infinite",)):
    """Inner multi-indices of the face (axis, side = -1 / +1) inside `area`."""
    its = b.inner_indices()
    its = its[its[:, axis] == (0 if side < 0 else b.sizes[axis] - 1)]
    X, Y, Z = b.coords(its)
    return its[O.area_contains(area, X, Y, Z)]


def apply_border(b, axis, side, nodes, values):
    """cubic::BorderConditions::handleBorderPoint (BorderConditions.hpp:94-114)
    on the acoustic vector: every ghost mirrors its inner node, then each named
    quantity becomes -inner + 2 f(t).  `values`: [(quantity name, f(t))] in the
    reference's map order."""
    sign = 1 if side < 0 else -1
    vals = sorted(values, key=lambda kv: O.QUANTITY_ORDER.index(kv[0]))
    for a in range(1, b.bs + 1):
        inner = nodes.copy(); inner[:, axis] += sign * a
        ghost = nodes.copy(); ghost[:, axis] -= sign * a
        fi, fg = b.flat_index(inner), b.flat_index(ghost)
        g = b.pde[fi].copy()
        for q, f in vals:
            j = quantity_index(b.D, q)
            g[:, j] = -b.pde[fi][:, j] + 2 * f
        b.pde[fg] = g


class Engine:
    """cubic::Engine<D> + AbstractEngine for ONE acoustic body: tau = Courant *
    min h / max eigenvalue (Engine.cpp:124-140), per step and axis border ->
    stage -> swap (Engine.cpp:90-121), the Clock of AbstractEngine::run.
    `ic_quantities`: [(area, quantity, value)]; `borders`: [(axis, area,
    {quantity: f(t)})], both faces of the axis as the reference applies them."""

    def __init__(self, D, bs, sizes, h, courant, rho, lam, ic_quantities=(), borders=(),
                 number_of_snaps=1, steps_per_snap=1):
        self.b = acoustic_body(D, bs, sizes, h=h, rho=rho, lam=lam)
        b = self.b
        its = b.inner_indices()
        X, Y, Z = b.coords(its)
        acc = np.zeros((len(its), b.M))
        for area, q, value in ic_quantities:
            v = np.zeros(b.M)
            v[quantity_index(D, q)] = value
            m = O.area_contains(area, X, Y, Z)
            acc[m] = acc[m] + v
        b.pde[b.flat_index(its)] = acc
        self.borders = []
        for axis, area, vals in borders:
            self.borders.append((axis, face_nodes(b, axis, -1, area), face_nodes(b, axis, 1, area), vals))
        self.courant = courant
        self.time = 0.0
        self.time_step = self.estimate_time_step()
        self.required_time = self.time_step * number_of_snaps * steps_per_snap
        self.steps_done = 0

    def estimate_time_step(self):
        b = self.b
        hmin = float(np.finfo(np.float64).max)
        for i in range(b.D):
            if hmin > b.h[i]:
                hmin = b.h[i]
        return self.courant * hmin / b.maximal_eigenvalue

    def next_time_step(self):
        b = self.b
        for s in range(b.D):
            for axis, left, right, vals in self.borders:
                if axis != s:
                    continue
                now = [(q, f(self.time)) for q, f in vals.items()]
                if len(left):
                    apply_border(b, s, -1, left, now)
                if len(right):
                    apply_border(b, s, 1, right, now)
            b.stage(s, self.time_step)

    def run(self, max_steps=None):
        while self.time < self.required_time:
            if max_steps is not None and self.steps_done >= max_steps:
                break
            self.time_step = self.estimate_time_step()
            self.next_time_step()
            self.steps_done += 1
            self.time += self.time_step
        return self.steps_done


def context_for(b, path=None, device=0):
    """An acoustic gcmx context holding the body's tables and state."""
    import gcm_amd
    ctx = gcm_amd.Context(b.D, b.bs, b.sizes[:b.D], start=b.start[:b.D], h=b.h[:b.D], device=device,
                          model="acoustic")
    U, U1, L = b.tables[0]
    ctx.set_materials(U[None], U1[None], L[None])
    ctx.upload(b.pde)
    if path is not None:
        ctx.set_path(path)
    return ctx
