"""One table of launches: every kernel instance family the step can run, at the
smallest shapes that reach it.  tests/test_gpu_poison.py, test_gpu_states.py
and test_gpu_nonfinite.py run all of them; tests/test_states_cpu.py takes the
material sets.

An entry knows how to build the oracle body (zero state: the caller fills it),
how both sides advance, what both sides compare (all nodes, or the inner nodes
where the one-pass face step keeps ghosts on the chip and where the Maxwell ODE
scales the stored stresses), and the kernel the profile must name, so that a
case cannot drift onto another instance unnoticed.

Both sides return, per step, the list of states to compare: one for a one-pass
step, one per stage for the per-stage paths.  Each is a grid [X(, Y(, Z)), M].

Names with the prefix "gp-" are the general-position twins of the homogeneous
isotropic entries: the same shape, marks and instance, on the material ISO_GP,
none of whose structural coefficients is a power of two or equals another (on
(4, 2, 1) every one is, and four of them equal the kernels' constants 0.5 and
1), at the time step courant_tau gives.  Their grid steps are H_GP, unequal, so
that each axis has Newton coefficients, Lagrange weights and floor(q) of its
own, wherever the instance admits that.  A UNI, HET or ZS instance of
k_step_tx2 does not: the dispatch takes one only when the three axes' tables
are bitwise equal (same_axis, kernels_xyz.hip), and the kernel then reads the
X axis' table for all three stages.  The twins of those entries take the equal
steps H_GP_EQ, which keeps them on their instance; tests/test_states_cpu.py
states which twin has which steps and what either medium separates."""
import copy

import numpy as np

from gcm_amd import PATH_GENERIC, PATH_SPLIT
from tests import acoustic_ref
from tests.helpers import context_for, oracle_body, random_materials
from tests.test_gpu_2d import FACE2_CASES, face_body2, faces_at2
from tests.test_gpu_faces import conditions_at, face_body, face_maps, faces_at, free, partial_body
from tests.test_gpu_ortho import H_A, ortho_body
from tests.test_gpu_ortho_het import het_body
from tests.test_gpu_plane_builds import ISO as ISO_GP
from tests.test_gpu_wide_access import MATS, TAU_HET

FREE_ALL = [(0, 0, free(0)), (1, 0, free(1)), (2, 0, free(2))]
FREE_YZ = [(1, 0, free(1)), (2, 0, free(2))]
H_ACOUSTIC = (0.5, 0.4, 0.3)
TAU0, TAU0_HET = (3.0,), (3.0, 0.7)  # Maxwell relaxation times, per material
ISO_DYADIC = (4.0, 2.0, 1.0)
# The general-position medium (see the header): ISO_GP on unequal steps.  At
# Courant 0.9 q = |L| tau / h is 0.643 / 0.288, 0.9 / 0.403, 0.409 / 0.183
# (P / S per axis); at Courant 1.5 floor(q) of the P waves is (1, 1, 0).
H_GP = (0.7, 0.5, 1.1)
H_GP_EQ = (H_GP[0],) * 3  # for the instances that take equal axes only
# 2-D: at Courant 1.5 floor(q) of the P waves is (1, 0); with a second step of
# 0.5 both floors are 1, and a mix-up of the axes' floors would not show
H_GP2 = (0.7, 1.1)


def courant_tau(b, courant=0.9):
    return courant * min(b.h[:b.D]) / b.maximal_eigenvalue


def courant15_tau(b):
    return courant_tau(b, 1.5)


# ------------------------------------------------------------ material sets --
# name -> body(bs, sizes) with that set's tables, and its Courant 0.9 time step

def _iso(bs, sizes, start=None, h=None, material=ISO_DYADIC):
    return oracle_body(3, bs, sizes, start=start, h=h, materials=(material,))


def _gp(bs, sizes, start=None, h=H_GP):
    return _iso(bs, sizes, start, h=h, material=ISO_GP)


def _iso_het(bs, sizes):
    b = oracle_body(3, bs, sizes, materials=MATS, courant=0.9)
    random_materials(b, seed=sum(sizes) + bs)
    return b


def _iso2d(bs, sizes, h=(1.0, 0.5), material=ISO_DYADIC):
    return oracle_body(2, bs, sizes, h=list(h), materials=(material,))


def _gp2d(bs, sizes):
    return _iso2d(bs, sizes, h=H_GP2, material=ISO_GP)


def _table2d(bs, sizes):
    """One structural zero of U made non-zero: off the isotropic structure."""
    b = _iso2d(bs, sizes)
    for t in b.tables:
        t[0][0][0, 4] = 1e-3
    return b


def _acoustic(bs, sizes, h=H_ACOUSTIC):
    """c = 2 and c rho = 3: no invariant V +- p / (c rho) of the impulse of
    tests/states.py (V = 1, 2, 3 and p = 4) is zero, so it spreads both ways."""
    return acoustic_ref.acoustic_body(3, bs, sizes, h=h, rho=1.5, lam=6.0)


def _iso_het2(bs, sizes, conds=None):
    """Two materials, random ids; `conds`: whole-face conditions (axis, side, values)."""
    b = partial_body(bs, sizes, [(a, s, ("infinite",), v) for a, s, v in conds or ()], materials=MATS[:2])
    random_materials(b, seed=sum(sizes) + bs)
    return b


def with_maxwell(body, tau0):
    """`body` with MaxwellViscosityOde on, as Body.apply_odes expects it."""
    assert len(tau0) == len(body.tables)
    body.odes, body.tau0 = ["MAXWELL_VISCOSITY"], list(tau0)
    return body


MATERIAL_SETS = {
    "iso": (_iso, lambda b: 0.9),
    "iso_het": (_iso_het, lambda b: TAU_HET),
    "ortho": (lambda bs, sizes: ortho_body(bs, sizes), courant_tau),
    "ortho_het": (lambda bs, sizes: het_body(bs, sizes), courant_tau),
    "iso2d": (_iso2d, lambda b: 0.45),
    "table2d": (_table2d, lambda b: 0.45),
    "acoustic": (_acoustic, courant_tau),
    "iso_gp": (_gp, courant_tau),
    "iso_gp_eq": (lambda bs, sizes: _gp(bs, sizes, h=H_GP_EQ), courant_tau),
    "iso2d_gp": (_gp2d, courant_tau),
}


def scaled_areas(conds, h):
    """The conditions of a face-map entry (MAP_64, MAP_1024: boxes in physical
    coordinates on unit steps) on steps `h`: every box bound times its axis' step."""
    out = []
    for axis, side, area, vals in conds:
        assert area[0] == "box"
        lo, hi = (tuple(v * s for v, s in zip(bound, h)) for bound in area[1:])
        out.append((axis, side, ("box", lo, hi), vals))
    return out


# ------------------------------------------------------------------ entries --

class Launch:
    """kind: "step" (gcmx_step, one pass), "faces" (gcmx_step_faces), "map"
    (gcmx_step_face_map: the body's conditions as per-node face maps), "ode"
    (gcmx_step_ode with `tau0` per material, whole-face conditions if `conds`;
    the ODE must ride in the step's stores), "stages" (gcmx_stage per axis on a
    forced path) or "slabs" (an in-process group).  `context`: the function that
    builds the gcmx context of a body (the elastic one of tests/helpers.py)."""

    def __init__(self, name, kind, make_body, tau, prefix, marks=(), absent=(), fma_tag=False, compare="all",
                 conds=None, faces_at=None, path=None, expect_path="fused", slabs=None, tau0=None,
                 context=context_for):
        self.name, self.kind, self.make_body, self._tau = name, kind, make_body, tau
        self.prefix = (prefix,) if isinstance(prefix, str) else tuple(prefix)
        self.marks, self.absent, self.fma_tag = tuple(marks), tuple(absent), fma_tag
        self.compare = "inner" if kind in ("faces", "map", "ode", "slabs") else compare
        self.conds, self._faces_at, self.slabs = conds, faces_at, slabs
        self.path, self.expect_path = path, expect_path  # forced kernel path, gcmx_last_step_path
        self.tau0, self.context = tau0, context
        assert (kind == "ode") == (tau0 is not None)
        self.has_faces = kind in ("faces", "map") or conds is not None

    def __repr__(self):
        return self.name

    def variant(self, name, marks, absent=()):
        """The same launch under another name, expected on another instance."""
        e = copy.copy(self)
        e.name, e.marks, e.absent = name, tuple(marks), tuple(absent)
        return e

    def faces(self, t):
        """The gcmx_step_faces argument at time t (None: no conditions)."""
        return self._faces_at(self.conds, t) if self.conds is not None else None

    def body(self):
        return self.make_body()

    def tau(self, body):
        return self._tau(body) if callable(self._tau) else self._tau

    def grid(self, body, arr):
        """The compared part of an all-nodes array, as a grid (a copy)."""
        if self.compare == "inner":
            return body.inner_view(np.asarray(arr).reshape(body.pde.shape)).copy()
        return np.asarray(arr).reshape(tuple(body.shape_all) + (body.M,)).copy()

    def node_of(self, body, inner_index):
        """Index of an inner node in the compared grid."""
        off = 0 if self.compare == "inner" else body.bs
        return tuple(int(i) + off for i in inner_index)

    def oracle_step(self, body, t):
        tau, out = self.tau(body), []
        for s in range(body.D):
            if self.has_faces:
                body.apply_border(s, t)
            body.stage(s, tau)
            if self.kind == "stages":
                out.append(self.grid(body, body.pde))
        if self.kind == "ode":
            assert body.odes and len(body.tau0) == len(self.tau0)
            body.apply_odes(tau)
        if self.kind != "stages":
            out.append(self.grid(body, body.pde))
        return out

    def start(self, body, fp):
        return Run(self, body, fp)

    def check_kernels(self, names, fp_fma):
        assert names, f"{self.name}: the profile names no kernel"
        for k in names:
            assert k.startswith(self.prefix), f"{self.name}: ran {k}, expected {' or '.join(self.prefix)}"
            for m in self.marks:
                assert m in k, f"{self.name}: ran {k}, expected an instance with '{m}'"
            for m in self.absent:
                assert m not in k, f"{self.name}: ran {k}, expected an instance without '{m}'"
            if self.fma_tag:
                assert ("FMA" in k) == fp_fma, f"{self.name}: ran {k} in the {'FMA' if fp_fma else 'exact'} build"


class Run:
    """The GPU side of one entry: its context(s) holding `body`'s state."""

    def __init__(self, launch, body, fp):
        import gcm_amd
        self.G, self.launch, self.body, self.tau = gcm_amd, launch, body, launch.tau(body)
        if launch.kind == "slabs":
            self.ctxs = self._slabs(body, launch.slabs)
        else:
            self.ctxs = [launch.context(body, path=launch.path)]
        for c in self.ctxs:
            c.fp_mode = fp
            c.profile(True)
        self.fp_fma = fp == gcm_amd.FP_FMA
        self.fmap = self.ctxs[0].face_map(face_maps(body, body.sizes)) if launch.kind == "map" else None

    def _slabs(self, body, widths):
        """X slabs of `body` as one in-process group, boundary-first schedule; each
        uploads its own inner planes (x ghosts zero: the exchange fills them)."""
        G, bs = self.G, body.bs
        U, U1, L = body.tables[0]
        whole = body.pde.reshape(tuple(body.shape_all) + (body.M,))
        out, x0 = [], 0
        for X in widths:
            c = G.Context(3, bs, [X] + body.sizes[1:], start=[x0, 0, 0], h=body.h[:3])
            c.set_materials(U[None], U1[None], L[None])
            part = np.zeros((X + 2 * bs,) + whole.shape[1:])
            part[bs:-bs] = whole[bs + x0:bs + x0 + X]
            c.upload(part)
            c.set_schedule(G.SCHED_BFIRST)
            out.append(c)
            x0 += X
        G.comm_init_local(out)
        return out

    def result(self):
        L, b = self.launch, self.body
        if L.kind != "slabs":
            return L.grid(b, self.ctxs[0].download())
        bs = b.bs
        parts = [c.download().reshape(tuple(c.shape_all) + (c.M,))[bs:-bs, bs:-bs, bs:-bs] for c in self.ctxs]
        return np.concatenate(parts, axis=0)

    def step(self, t):
        L, c = self.launch, self.ctxs[0]
        if L.kind == "stages":
            out = []
            for s in range(self.body.D):
                c.stage(s, self.tau)
                assert c.last_path == L.expect_path, f"{L.name}: stage {s} ran {c.last_path}"
                out.append(self.result())
            return out
        if L.kind == "slabs":
            self.G.local_group_steps(self.ctxs, self.tau, 1)
        elif L.kind == "faces":
            c.step_faces(self.tau, L.faces(t))
        elif L.kind == "map":
            c.step_face_map(self.tau, self.fmap, conditions_at(self.body, t))
        elif L.kind == "ode":
            c.step_ode(self.tau, list(L.tau0), faces=L.faces(t))
            assert c.last_ode_fused, f"{L.name}: the ODE ran as a pass of its own"
        else:
            c.step(self.tau)
        for x in self.ctxs:
            assert x.last_path == L.expect_path, f"{L.name}: ran {x.last_path}"
        return [self.result()]

    def kernels(self):
        """The step kernels the profile names (helper buckets -- face fills, halo
        copies -- carry no kernel name)."""
        return [v["kernel"] for c in self.ctxs for v in c.profile_read().values() if v["launches"] > 0 and v["kernel"]]

    def check_kernels(self):
        names = self.kernels()
        self.launch.check_kernels(names, self.fp_fma)
        return names

    def close(self):
        if self.fmap is not None:
            self.fmap.close()
        for c in self.ctxs:
            c.close()


def _tx2(name, bs, sizes, path, start=None, gp=None, **kw):
    """path: "wide" (16-byte accesses), "n8" (a UNI launch on the 8-byte path) or
    "!uni" (idle lanes: the 8-byte instances).  gp: the steps of a general-position
    twin (ISO_GP at Courant 0.9)."""
    marks = {"wide": (", UNI",), "n8": (", UNI", ", N8"), "!uni": ("!UNI",)}[path]
    absent = {"wide": (", N8",), "n8": (), "!uni": ()}[path]
    make, tau = (lambda: _iso(bs, sizes, start), 0.9) if gp is None else \
        (lambda: _gp(bs, sizes, start, h=gp), courant_tau)
    return Launch(name, "step", make, tau, f"k_step_tx2<{bs}, ", marks + kw.pop("marks", ()), absent, fma_tag=True,
                  **kw)


def _het(name, bs, sizes, path):
    marks = {"wide": (", UNI", ", HET"), "n8": (", UNI", ", HET", ", N8")}[path]
    return Launch(name, "step", lambda: _iso_het(bs, sizes), TAU_HET, f"k_step_tx2<{bs}, ", marks,
                  (", N8",) if path == "wide" else (), fma_tag=True)


def _stages(name, sizes, path_name, make=_iso, tau=0.9):
    path = {"split": PATH_SPLIT, "generic": PATH_GENERIC}[path_name]
    prefix = {"split": ("k_march<", "k_line_z"), "generic": ("k_stage_generic",)}[path_name]
    return Launch(name, "stages", lambda: make(2, sizes), tau, prefix, path=path, expect_path=path_name)


def _ortho(name, bs, sizes, h=H_A, tau=courant_tau, marks=(", KF0",)):
    return Launch(name, "step", lambda: ortho_body(bs, sizes, h=h), tau, f"k_step_ortho<{bs}, ", marks,
                  (", HET",), fma_tag=True)


# Face entries take free surfaces (every prescribed value 0): the step stays
# linear and homogeneous, which the impulse footprints and the power-of-two
# scaling of tests/test_gpu_states.py rest on.
def _face2d(gp=False):
    bs, sizes, conds, courant, path = FACE2_CASES["free_all"]
    assert path == "fused"
    if gp:
        make = lambda: face_body2(bs, sizes, conds, h=H_GP2, material=ISO_GP)
        return Launch("gp-2d-faces-free4-30x70", "faces", make, courant_tau, "k_step2d_iso<2, ", (", FACES",),
                      conds=conds, faces_at=faces_at2)
    return Launch("2d-faces-free4-30x70", "faces", lambda: face_body2(bs, sizes, conds), courant, "k_step2d_iso<2, ",
                  (", FACES",), conds=conds, faces_at=faces_at2)


def _gp_faces(bs, sizes, conds=FREE_ALL, h=H_GP):
    return lambda: face_body(3, bs, sizes, conds, h=h, material=ISO_GP)


def _faces3(name, bs, sizes, marks, conds=FREE_ALL, tau=0.9, make_body=None, prefix=None, absent=("!FACES",)):
    """gcmx_step_faces with whole-face conditions (free surfaces on every face
    unless `conds` says otherwise)."""
    return Launch(name, "faces", make_body or (lambda: face_body(3, bs, sizes, conds)), tau,
                  prefix or f"k_step_tx2<{bs}, ", marks, absent, fma_tag=True, conds=conds,
                  faces_at=lambda c, t: faces_at(3, c, t))


def _ode(name, bs, make_body, tau0, marks, tau=0.9, conds=None, absent=()):
    """gcmx_step_ode, the ODE folded into the pass (asserted per step)."""
    return Launch(name, "ode", lambda: with_maxwell(make_body(), tau0), tau, f"k_step_tx2<{bs}, ", marks, absent,
                  fma_tag=True, tau0=tau0, conds=conds, faces_at=lambda c, t: faces_at(3, c, t))


def _map(name, bs, sizes, conds, marks, gp=None):
    """gcmx_step_face_map; conds: (axis, side or 0, area, values) of partial_body.
    gp: the steps of a general-position twin, whose areas are `conds` scaled."""
    make, tau = (lambda: partial_body(bs, sizes, conds), 0.9) if gp is None else \
        (lambda: partial_body(bs, sizes, scaled_areas(conds, gp), materials=(ISO_GP,), h=gp), courant_tau)
    return Launch(name, "map", make, tau, f"k_step_tx2<{bs}, ", marks, ("!FACES",), fma_tag=True)


def _acoustic_launch(name, bs, sizes, zt, h=H_ACOUSTIC, tau=courant_tau, kf0="KF0"):
    """The fp mode changes nothing on acoustic contexts: no FMA tag to expect."""
    return Launch(name, "step", lambda: _acoustic(bs, sizes, h=h), tau, f"k_step_acoustic<{bs}, {zt}, {kf0}>",
                  context=acoustic_ref.context_for)


_zero = lambda t: 0.0
# half of y- free, both z faces free on a box of x and y, no condition (zero
# ghosts) on the rest of those faces and on every other face
MAP_64 = [(1, -1, ("box", (-1, -1, -1), (2.5, 1, 100)), free(1)),
          (2, 0, ("box", (0.5, 2.5, -100), (100, 8.5, 2000)), free(2))]
# rows of 1024: partial y faces across the cut columns (z 508 .. 515), ending on
# the cut, and on both parts; part of z+ held fixed in the last part
MAP_1024 = [(1, -1, ("box", (-1, -1, 300.5), (100, 1, 700.5)), free(1)),
            (1, 1, ("box", (1.5, 8, -1), (100, 100, 511.5)), free(1)),
            (2, 1, ("box", (-1, 3.5, -100), (100, 7.5, 2000)), {"Vz": _zero, "Sxz": _zero})]

CATALOG = [
    # ---- k_step_tx2
    _tx2("tx2-wide-bs2-4x5x64", 2, [4, 5, 64], "wide"),
    _tx2("tx2-wide-bs2-3x6x128", 2, [3, 6, 128], "wide"),
    _tx2("tx2-wide-bs1-4x5x64", 1, [4, 5, 64], "wide"),
    _tx2("tx2-wide-start1-bs2-4x5x64", 2, [4, 5, 64], "wide", start=[1, 0, 0]),
    _tx2("tx2-n8-bs2-3x6x256", 2, [3, 6, 256], "n8"),
    _tx2("tx2-!uni-bs2-4x6x40", 2, [4, 6, 40], "!uni"),
    _tx2("tx2-zs-bs2-4x12x1024", 2, [4, 12, 1024], "wide", marks=(", ZS",)),
    _het("tx2-het-bs1-5x7x64", 1, [5, 7, 64], "wide"),
    _het("tx2-het-bs2-4x6x128", 2, [4, 6, 128], "n8"),
    Launch("tx2-faces-free6-bs2-4x8x64", "faces", lambda: face_body(3, 2, [4, 8, 64], FREE_ALL), 0.9,
           "k_step_tx2<2, ", (", UNI", ", FACES"), ("!FACES", ", N8"), fma_tag=True, conds=FREE_ALL,
           faces_at=lambda conds, t: faces_at(3, conds, t)),
    # floor(q) = 1 on the fast waves: whichever of the two kernels the dispatch
    # takes (k_step_tx2's !KF0 instance at this border size; see the profile)
    Launch("courant15-bs2-4x6x64", "step", lambda: _iso(2, [4, 6, 64]), 1.5, ("k_step_tx2<2, ", "k_fused_xyz<2, "),
           ("!KF0",), fma_tag=True),
    # ---- k_step_tx2 with faces beyond the UNI bs 2 instance; per-node face maps
    _faces3("tx2-zs-faces-free6-bs2-4x12x1024", 2, [4, 12, 1024], (", UNI", ", FACES", ", ZS"),
            prefix="k_step_tx2<2, 512, KF0, "),
    _faces3("tx2-zs-faces-free6-bs1-4x8x1024", 1, [4, 8, 1024], (", UNI", ", FACES", ", ZS"),
            prefix="k_step_tx2<1, 512, KF0, "),
    _faces3("tx2-het-faces-free6-bs2-4x8x64", 2, [4, 8, 64], (", UNI", ", FACES", ", HET"), tau=TAU_HET,
            make_body=lambda: _iso_het2(2, [4, 8, 64], FREE_ALL)),
    _faces3("tx2-faces-!uni-free6-bs2-4x8x40", 2, [4, 8, 40], ("!UNI", ", FACES")),
    _faces3("tx2-faces-free6-bs1-4x6x64", 1, [4, 6, 64], (", FACES",)),
    # floor(q) = 1 on the fast waves, y and z faces free (no x face: the x ghosts
    # are the state's own)
    _faces3("tx2-faces-courant15-bs2-4x8x64", 2, [4, 8, 64], ("!KF0", ", FACES"), conds=FREE_YZ, tau=1.5),
    _map("tx2-map-bs2-6x12x64", 2, [6, 12, 64], MAP_64, (", FACES",)),
    _map("tx2-map-zs-bs2-4x10x1024", 2, [4, 10, 1024], MAP_1024, (", FACES", ", ZS")),
    # ---- the Maxwell ODE folded into the pass: one factor, per-node factors, with
    # faces, and in both kernels of the z split
    _ode("tx2-ode-bs2-4x6x64", 2, lambda: _iso(2, [4, 6, 64]), TAU0, ("<2, 64, ",)),
    _ode("tx2-het-ode-bs1-5x7x64", 1, lambda: _iso_het2(1, [5, 7, 64]), TAU0_HET, (", HET",), tau=TAU_HET),
    _ode("tx2-faces-ode-bs2-4x8x64", 2, lambda: face_body(3, 2, [4, 8, 64], FREE_ALL), TAU0, (", UNI", ", FACES"),
         conds=FREE_ALL, absent=("!FACES", ", N8")),
    _ode("tx2-zs-ode-bs2-4x12x1024", 2, lambda: _iso(2, [4, 12, 1024]), TAU0, (", UNI", ", ZS")),
    # ---- k_step_acoustic (M = D + 1; its own stage code and limiter)
    _acoustic_launch("acoustic-bs2-4x5x64", 2, [4, 5, 64], 64),
    _acoustic_launch("acoustic-bs1-6x9x37", 1, [6, 9, 37], 64),
    _acoustic_launch("acoustic-bs3-5x7x20", 3, [5, 7, 20], 64),
    # floor(q) = 1: tau = h / c (c = 2), Courant 1 on a unit grid
    _acoustic_launch("acoustic-!kf0-bs2-6x9x37", 2, [6, 9, 37], 64, h=(1.0, 1.0, 1.0), tau=0.5, kf0="!KF0"),
    # rows with a wave seam and idle lanes
    _acoustic_launch("acoustic-bs2-3x5x130", 2, [3, 5, 130], 256),
    # ---- other 3-D paths
    Launch("fused_xyz-bs3-4x7x100", "step", lambda: _iso(3, [4, 7, 100]), 0.9, "k_fused_xyz<3, ", fma_tag=True),
    _stages("split-bs2-9x4x300", [9, 4, 300], "split"),
    _stages("generic-bs2-5x6x70", [5, 6, 70], "generic"),
    _ortho("ortho-bs2-6x9x37", 2, [6, 9, 37]),
    _ortho("ortho-bs2-4x5x65", 2, [4, 5, 65]),
    _ortho("ortho-bs3-5x7x20", 3, [5, 7, 20]),
    _ortho("ortho-!kf0-bs2-6x9x37", 2, [6, 9, 37], h=(1.0, 1.0, 1.0), tau=0.158, marks=("!KF0",)),
    Launch("ortho-het-bs2-6x9x37", "step", lambda: het_body(2, [6, 9, 37]), courant_tau, "k_step_ortho<2, ",
           (", KF0", ", HET"), fma_tag=True),
    Launch("slabs-bfirst-bs2-8+8x6x64", "slabs", lambda: _iso(2, [16, 6, 64]), 0.9, "k_step_tx2<2, ", fma_tag=True,
           slabs=(8, 8)),
    # ---- 2-D
    Launch("2d-iso-bs2-21x70", "step", lambda: _iso2d(2, [21, 70]), 0.45, "k_step2d_iso<2, "),
    Launch("2d-iso-bs1-130x253", "step", lambda: _iso2d(1, [130, 253]), 0.45, "k_step2d_iso<1, "),
    Launch("2d-table-bs2-30x300", "step", lambda: _table2d(2, [30, 300]), 0.45, "k_step2d<2, "),
    _face2d(),
]

# The general-position twins (see the header).  EQ: the entry's instance takes
# bitwise-equal axes only (UNI, ZS), so its twin has equal steps.
EQ = H_GP_EQ
CATALOG += [
    # ---- k_step_tx2
    _tx2("gp-tx2-wide-bs2-4x5x64", 2, [4, 5, 64], "wide", gp=EQ),
    _tx2("gp-tx2-wide-bs2-3x6x128", 2, [3, 6, 128], "wide", gp=EQ),
    _tx2("gp-tx2-wide-bs1-4x5x64", 1, [4, 5, 64], "wide", gp=EQ),
    _tx2("gp-tx2-wide-start1-bs2-4x5x64", 2, [4, 5, 64], "wide", start=[1, 0, 0], gp=EQ),
    _tx2("gp-tx2-n8-bs2-3x6x256", 2, [3, 6, 256], "n8", gp=EQ),
    _tx2("gp-tx2-!uni-bs2-4x6x40", 2, [4, 6, 40], "!uni", gp=H_GP),
    _tx2("gp-tx2-zs-bs2-4x12x1024", 2, [4, 12, 1024], "wide", marks=(", ZS",), gp=EQ),
    # ---- floor(q) of the P waves (1, 1, 0), of the S waves 0
    Launch("gp-courant15-bs2-4x6x64", "step", lambda: _gp(2, [4, 6, 64]), courant15_tau,
           ("k_step_tx2<2, ", "k_fused_xyz<2, "), ("!KF0",), fma_tag=True),
    _faces3("gp-tx2-faces-courant15-bs2-4x8x64", 2, [4, 8, 64], ("!KF0", ", FACES"), conds=FREE_YZ, tau=courant15_tau,
            make_body=_gp_faces(2, [4, 8, 64], FREE_YZ)),
    # ---- faces
    _faces3("gp-tx2-faces-free6-bs2-4x8x64", 2, [4, 8, 64], (", UNI", ", FACES"), tau=courant_tau,
            make_body=_gp_faces(2, [4, 8, 64], h=EQ), absent=("!FACES", ", N8")),
    _faces3("gp-tx2-zs-faces-free6-bs2-4x12x1024", 2, [4, 12, 1024], (", UNI", ", FACES", ", ZS"), tau=courant_tau,
            make_body=_gp_faces(2, [4, 12, 1024], h=EQ), prefix="k_step_tx2<2, 512, KF0, "),
    _faces3("gp-tx2-zs-faces-free6-bs1-4x8x1024", 1, [4, 8, 1024], (", UNI", ", FACES", ", ZS"), tau=courant_tau,
            make_body=_gp_faces(1, [4, 8, 1024], h=EQ), prefix="k_step_tx2<1, 512, KF0, "),
    _faces3("gp-tx2-faces-!uni-free6-bs2-4x8x40", 2, [4, 8, 40], ("!UNI", ", FACES"), tau=courant_tau,
            make_body=_gp_faces(2, [4, 8, 40])),
    # unequal axes: the !UNI instance on whole waves (the original runs a UNI one)
    _faces3("gp-tx2-faces-free6-bs1-4x6x64", 1, [4, 6, 64], (", FACES",), tau=courant_tau,
            make_body=_gp_faces(1, [4, 6, 64])),
    # ---- maps, their areas scaled to the steps
    _map("gp-tx2-map-bs2-6x12x64", 2, [6, 12, 64], MAP_64, (", FACES",), gp=H_GP),
    _map("gp-tx2-map-zs-bs2-4x10x1024", 2, [4, 10, 1024], MAP_1024, (", FACES", ", ZS"), gp=EQ),
    # ---- the folded ODE
    _ode("gp-tx2-ode-bs2-4x6x64", 2, lambda: _gp(2, [4, 6, 64]), TAU0, ("<2, 64, ",), tau=courant_tau),
    _ode("gp-tx2-faces-ode-bs2-4x8x64", 2, _gp_faces(2, [4, 8, 64], h=EQ), TAU0, (", UNI", ", FACES"), tau=courant_tau,
         conds=FREE_ALL, absent=("!FACES", ", N8")),
    _ode("gp-tx2-zs-ode-bs2-4x12x1024", 2, lambda: _gp(2, [4, 12, 1024], h=EQ), TAU0, (", UNI", ", ZS"),
         tau=courant_tau),
    # ---- other 3-D paths; the second slab starts on an odd global plane
    Launch("gp-fused_xyz-bs3-4x7x100", "step", lambda: _gp(3, [4, 7, 100]), courant_tau, "k_fused_xyz<3, ",
           fma_tag=True),
    _stages("gp-split-bs2-9x4x300", [9, 4, 300], "split", make=_gp, tau=courant_tau),
    Launch("gp-slabs-bfirst-bs2-7+9x6x64", "slabs", lambda: _gp(2, [16, 6, 64]), courant_tau, "k_step_tx2<2, ",
           fma_tag=True, slabs=(7, 9)),
    # ---- 2-D; mixed: floor(q) of the P waves (1, 0)
    Launch("gp-2d-iso-bs2-21x70", "step", lambda: _gp2d(2, [21, 70]), courant_tau, "k_step2d_iso<2, "),
    Launch("gp-2d-iso-bs1-130x253", "step", lambda: _gp2d(1, [130, 253]), courant_tau, "k_step2d_iso<1, "),
    _face2d(gp=True),
    Launch("gp-2d-iso-mixed-bs2-21x70", "step", lambda: _gp2d(2, [21, 70]), courant15_tau, "k_step2d_iso<2, ",
           ("!KF0",)),
]
BY_NAME = {e.name: e for e in CATALOG}
# twin -> original (the slab twin splits 7 + 9 where the original splits 8 + 8,
# and the mixed-floor 2-D entry has no original)
TWINS = {n: n[len("gp-"):] for n in BY_NAME if n.startswith("gp-") and n[len("gp-"):] in BY_NAME}
assert len(BY_NAME) == len(CATALOG)
