"""The step dispatch as a table: per case a context and a short script of ABI
calls, and after each call what the library answered -- status, effective
path, last path, whether the ODE was folded, the profile's buckets and kernel
names, and (exact build) the SHA-256 of the downloaded state.

tests/golden/step_plan.json holds these records as a library built from the
commit BEFORE the step planner (gcm_amd/csrc/plan.hpp) gave them;
tests/test_gpu_step_plan.py asserts the current library reproduces them
exactly.  Each step call also names the StepPlan (plan.hpp) it expects:
tests/test_plan_cpu.py checks that these cover every plan the planner can
return.

Recording (never run by pytest; refuses to overwrite without --force):

    GCMX_LIB=<library of the commit to record> python -m tests.step_plan_table --record
"""
import hashlib
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan.json")
SEED = 0x5EED
Q = {"Vx": 2, "Vy": 3, "Vz": 4, "Sxx": 5, "Sxy": 6, "Sxz": 7, "Syy": 8, "Syz": 9, "Szz": 10, "PRESSURE": 12}
FREE3 = {0: ("Sxx", "Sxy", "Sxz"), 1: ("Syy", "Sxy", "Syz"), 2: ("Szz", "Sxz", "Syz")}
FREE2 = {0: ("Sxx", "Sxy"), 1: ("Syy", "Sxy")}
H_A = (0.5, 0.4, 0.3)
ISO_MATS = ((4.0, 2.0, 1.0), (1.0, 2.0, 0.8))  # (rho, lambda, mu); the second is the faster: c1 = sqrt(3.6)


# ------------------------------------------------------------------- media --
# name -> (model, D, h, tables [(U, U1, L)], per-node ids?, unit tau: Courant 1 on the fastest wave)

def _max_l(tabs, h):
    return max(float(np.abs(L[s]).max()) / h[s] for _, _, L in tabs for s in range(L.shape[0]))


def medium(name):
    from oracle import oracle as O
    from tests import acoustic_ref as A
    from tests.test_ortho_cpu import MAT_A, MAT_B, ortho_tables
    if name == "iso":
        return "elastic", 3, (1.0, 1.0, 1.0), [O.isotropic_elastic_matrices(3, *ISO_MATS[0])], False
    if name == "iso_het":
        return "elastic", 3, (1.0, 1.0, 1.0), [O.isotropic_elastic_matrices(3, *m) for m in ISO_MATS], True
    if name == "general":  # one structural zero of U made non-zero: no pattern matches
        U, U1, L = (a.copy() for a in O.isotropic_elastic_matrices(3, *ISO_MATS[0]))
        assert U[0, 0, 4] == 0.0
        U[0, 0, 4] = 1e-3
        return "elastic", 3, (1.0, 1.0, 1.0), [(U, U1, L)], False
    if name == "ortho":
        return "elastic", 3, H_A, [ortho_tables(*MAT_A)], False
    if name == "ortho_het":
        return "elastic", 3, H_A, [ortho_tables(*MAT_A), ortho_tables(*MAT_B)], True
    if name == "acoustic":
        return "acoustic", 3, H_A, [A.acoustic_tables(3, 2.0, 8.0)], False
    if name == "iso2d":
        return "elastic", 2, (1.0, 0.5), [O.isotropic_elastic_matrices(2, *ISO_MATS[0])], False
    if name == "table2d":
        U, U1, L = (a.copy() for a in O.isotropic_elastic_matrices(2, *ISO_MATS[0]))
        assert U[0, 0, 4] == 0.0
        U[0, 0, 4] = 1e-3
        return "elastic", 2, (1.0, 0.5), [(U, U1, L)], False
    raise KeyError(name)


# ------------------------------------------------------------------- calls --
# (op, argument, tau as a Courant number or None, expected plan or None)

def step(plan, courant=0.9):
    return ("step", None, courant, plan)


def faces(which, plan, courant=0.9):
    """which: "free" (every face free), "ypressure" (y- sets PRESSURE), "pressure" (acoustic: all faces p = 0)."""
    return ("faces", which, courant, plan)


def ode(plan, with_faces=None, courant=0.9):
    return ("ode", with_faces, courant, plan)


def fmap(which, plan, courant=0.9):
    """which: "mixed" (y-: two conditions, node by node) or "uniform" (y-: one condition)."""
    return ("map", which, courant, plan)


def stage(axis, courant=0.9):
    return ("stage", axis, courant, None)


QUERY = ("query", None, None, None)
BORDER_FILL = ("border_fill", None, None, None)


def path(p):
    return ("path", p, None, None)


STAGES3 = [stage(0), stage(1), stage(2)]
PATHS = [x for p in ("generic", "split", "fused", "auto") for x in (path(p), QUERY, step(None))]
# the plan of the step after each forced path, per medium
ST, TX2, ORTHO, AC, S2D = "Stages - -", "Tx2 - -", "Ortho - -", "Acoustic - -", "Step2d - -"


def forced(plans):
    """PATHS with the expected plans of its four steps (generic, split, fused, auto)."""
    it = iter(plans)
    return [(op, a, c, next(it)) if op == "step" else (op, a, c, p) for op, a, c, p in PATHS]


class Case:
    def __init__(self, name, medium, bs, sizes, script, slabs=None):
        self.name, self.medium, self.bs, self.sizes, self.script, self.slabs = name, medium, bs, sizes, script, slabs

    def __repr__(self):
        return self.name


CASES = [
    # ---- Iso3: k_step_tx2 / k_fused_xyz
    # Y = 5 < 2 bs + 2: the face step takes the stages, and its written faces keep the next plain step there
    Case("iso-wide-bs2-4x5x64", "iso", 2, [4, 5, 64], [QUERY, step(TX2), faces("free", ST), QUERY, step(ST)]),
    Case("iso-wide-bs1-4x5x64", "iso", 1, [4, 5, 64],
         [step(TX2), ode("Tx2 - ode"), ode("Tx2 faces ode", with_faces="free"), faces("free", "Tx2 faces -")]),
    Case("iso-n8-bs2-3x6x256", "iso", 2, [3, 6, 256],
         [step(TX2), faces("free", "Tx2 faces -"), QUERY, step(ST), faces("free", "Tx2 faces -")]),
    Case("iso-!uni-bs2-4x6x40", "iso", 2, [4, 6, 40],
         [step(TX2), fmap("mixed", "Tx2 faces -"), fmap("uniform", "Tx2 faces -"), faces("ypressure", ST),
          ode(ST, with_faces="ypressure")]),
    # rows of 1024: the z split carries faces and the ODE; at floor(q) = 1 it does not run
    Case("iso-zs-bs2-4x12x1024", "iso", 2, [4, 12, 1024],
         [step(TX2), ode("Tx2 - ode"), faces("free", "Tx2 faces -")]),
    Case("iso-zs-courant15-bs2-4x12x1024", "iso", 2, [4, 12, 1024],
         [step(TX2, 1.5), ode(TX2, courant=1.5), faces("free", ST, 1.5)]),
    Case("iso-fused_xyz-bs3-4x7x100", "iso", 3, [4, 7, 100], [step(TX2), ode(TX2), faces("free", ST)]),
    Case("iso-courant15-bs2-4x6x64", "iso", 2, [4, 6, 64], [step(TX2, 1.5), ode("Tx2 - ode", courant=1.5)]),
    Case("iso-ghosts-bs2-4x6x64", "iso", 2, [4, 6, 64], [step(TX2), BORDER_FILL, QUERY, step(ST), faces("free", ST)]),
    Case("iso-paths-bs2-4x6x64", "iso", 2, [4, 6, 64], forced([ST, ST, TX2, TX2])),
    Case("iso-stages-bs2-4x6x64", "iso", 2, [4, 6, 64], STAGES3 + [step(TX2)]),
    Case("iso-slabs-bs2-8+8x6x64", "iso", 2, [16, 6, 64], [step(TX2), step(TX2)], slabs=(8, 8)),
    # ---- IsoHet: k_step_tx2 HET
    Case("het-bs1-5x7x64", "iso_het", 1, [5, 7, 64],
         [QUERY, step(TX2), ode("Tx2 - ode"), ode("Tx2 faces ode", with_faces="free"), QUERY, step(ST)]),
    # floor(q) = 1: tau_ok is lost (the query does not see it), and comes back with the next tau
    Case("het-bs2-4x6x128", "iso_het", 2, [4, 6, 128],
         [step(TX2), step(ST, 1.5), QUERY, ode(ST, courant=1.5), step(TX2), fmap("mixed", "Tx2 faces -"),
          faces("ypressure", ST)]),
    Case("het-paths-bs2-4x6x128", "iso_het", 2, [4, 6, 128], forced([ST, ST, TX2, TX2]) + STAGES3 + [BORDER_FILL, QUERY, step(ST)]),
    # ---- Ortho: k_step_ortho
    Case("ortho-bs2-6x9x37", "ortho", 2, [6, 9, 37],
         [QUERY, step(ORTHO), ode(ORTHO), faces("free", ST), QUERY, step(ST)]),
    Case("ortho-tau-bs2-6x9x37", "ortho", 2, [6, 9, 37],
         [step(ORTHO, 1.5), step(ST, -0.9), QUERY, step(ORTHO), fmap("uniform", ST)]),
    Case("ortho-bs3-5x7x20", "ortho", 3, [5, 7, 20], [step(ORTHO)] + STAGES3 + [step(ORTHO)]),
    Case("ortho-paths-bs2-6x9x37", "ortho", 2, [6, 9, 37], forced([ST, ST, ORTHO, ORTHO]) + [BORDER_FILL, QUERY, step(ST)]),
    Case("ortho-slabs-bs2-8+8x6x37", "ortho", 2, [16, 6, 37], [step(ORTHO), step(ORTHO)], slabs=(8, 8)),
    # ---- OrthoHet: k_step_ortho HET
    Case("orthohet-bs2-6x9x37", "ortho_het", 2, [6, 9, 37],
         [QUERY, step(ORTHO), ode(ORTHO), step(ST, 1.5), QUERY, step(ORTHO), step(ST, -0.9), faces("free", ST), QUERY,
          step(ST)]),
    Case("orthohet-paths-bs2-6x9x37", "ortho_het", 2, [6, 9, 37], forced([ST, ST, ORTHO, ORTHO]) + STAGES3),
    # ---- Acoustic: k_step_acoustic
    Case("acoustic-bs1-6x9x37", "acoustic", 1, [6, 9, 37], [QUERY, step(AC), faces("pressure", ST), QUERY, step(ST)]),
    Case("acoustic-bs2-4x2x4", "acoustic", 2, [4, 2, 4],
         [step(AC), step(AC, 1.5), step(ST, -0.9), QUERY, step(AC), ode(None), fmap("uniform", ST)]),
    Case("acoustic-bs3-5x7x20", "acoustic", 3, [5, 7, 20], [step(AC)] + STAGES3 + [BORDER_FILL, QUERY, step(ST)]),
    Case("acoustic-paths-bs2-4x2x4", "acoustic", 2, [4, 2, 4], forced([ST, ST, AC, AC])),
    # ---- 2-D: k_step2d
    Case("2d-iso-bs2-21x70", "iso2d", 2, [21, 70],
         [QUERY, step(S2D), ode(S2D), faces("free", "Step2d faces -"), QUERY, step(ST), faces("free", "Step2d faces -"),
          faces("ypressure", ST), fmap("uniform", ST)]),
    Case("2d-iso-bs2-30x70", "iso2d", 2, [30, 70],
         [ode("Step2d faces -", with_faces="free"), stage(0), stage(1), BORDER_FILL, QUERY, step(ST)]),
    Case("2d-iso-paths-bs2-21x70", "iso2d", 2, [21, 70], forced([ST, ST, S2D, S2D])),
    Case("2d-table-bs2-30x70", "table2d", 2, [30, 70], [QUERY, step(S2D), faces("free", ST), QUERY, step(ST)]),
    # ---- General: the stages
    Case("general-bs2-5x6x70", "general", 2, [5, 6, 70],
         [QUERY, step(ST), faces("free", ST), ode(ST), fmap("mixed", ST)] + STAGES3 + forced([ST, ST, ST, ST])),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def expected_plans():
    """Every plan the table's step calls name."""
    return sorted({p for c in CASES for _, _, _, p in c.script if p is not None})


# ------------------------------------------------------------------ running --

def _faces_arg(which, D, model):
    if which == "pressure":
        return [[(Q["PRESSURE"], 0.0)] for _ in range(2 * D)]
    free = FREE3 if D == 3 else FREE2
    out = [[(Q[q], 0.0) for q in free[f // 2]] for f in range(2 * D)]
    if which == "ypressure":
        out[2] = [(Q["PRESSURE"], 0.5)]
    return out


def _contexts(G, case, fp):
    model, D, h, tabs, ids = medium(case.medium)
    U, U1, L = (np.stack([t[i] for t in tabs]) for i in range(3))
    out, x0 = [], 0
    for X in case.slabs or (case.sizes[0],):
        sizes = [X] + case.sizes[1:]
        c = G.Context(D, case.bs, sizes, start=[x0] + [0] * (D - 1), h=h[:D], model=model)
        c.set_materials(U, U1, L)
        if ids:
            rng = np.random.default_rng(sum(sizes) + case.bs)
            c.set_material_ids(rng.integers(0, len(tabs), c.n_all).astype(np.uint8))
        c.fp_mode = fp
        c.fill_random(case.sizes, SEED)
        if case.slabs:
            c.set_schedule(G.SCHED_BFIRST)
        c.profile(True)
        out.append(c)
        x0 += X
    if case.slabs:
        G.comm_init_local(out)
    return out, _max_l(tabs, h), D, model, len(tabs)


def _map_for(c, D, which):
    n = int(np.prod([s for d, s in enumerate(c.sizes) if d != 1]))
    m = np.zeros(n, dtype=np.uint8)
    if which == "mixed":
        m[n // 2:] = 1
    return c.face_map([None, None, m] + [None] * (2 * D - 3))


def run_case(G, case, fp):
    """The records of one case: one per call and context."""
    ctxs, max_l, D, model, n_mat = _contexts(G, case, fp)
    exact = fp == G.FP_EXACT
    records = []
    maps = {}
    for op, arg, courant, _ in case.script:
        tau = None if courant is None else courant / max_l
        for c in ctxs:
            c.profile_reset()
        status = 0
        try:
            c = ctxs[0]
            if op == "step" and case.slabs:
                G.local_group_steps(ctxs, tau, 1)
            elif op == "step":
                c.step(tau)
            elif op == "faces":
                c.step_faces(tau, _faces_arg(arg, D, model))
            elif op == "ode":
                c.step_ode(tau, [0.7 + 0.2 * m for m in range(n_mat)], faces=None if arg is None else _faces_arg(arg, D, model))
            elif op == "map":
                if arg not in maps:
                    maps[arg] = _map_for(c, D, arg)
                free = FREE3 if D == 3 else FREE2
                conds = [[(Q[q], 0.0) for q in free[1]], [(Q["Vy"], 0.25)]]
                if model == "acoustic":
                    conds = [[(Q["PRESSURE"], 0.0)], [(Q["Vy"], 0.25)]]
                c.step_face_map(tau, maps[arg], conds)
            elif op == "stage":
                c.stage(arg, tau)
            elif op == "border_fill":
                c.border_fill(1, -1, np.zeros((1, D), dtype=np.int32), [Q["Vy"]], [0.0])
            elif op == "path":
                c.set_path({"auto": G.PATH_AUTO, "generic": G.PATH_GENERIC, "split": G.PATH_SPLIT, "fused": G.PATH_FUSED}[arg])
            else:
                assert op == "query", op
        except G.GcmxError as e:
            status = e.status
        for c in ctxs:
            c.sync()
            prof = c.profile_read()
            rec = {"status": status, "effective_path": c.effective_path, "last_path": c.last_path,
                   "ode_fused": c.last_ode_fused,
                   "kernels": [f"{b}:{v['kernel']}" for b, v in prof.items() if v["launches"] > 0]}
            if exact:
                rec["sha256"] = hashlib.sha256(np.ascontiguousarray(c.download()).tobytes()).hexdigest()
            records.append(rec)
    for c in ctxs:
        c.close()
    return records


def run_all(G):
    return {f"{case.name}/{name}": run_case(G, case, fp)
            for case in CASES for name, fp in (("fma", G.FP_FMA), ("exact", G.FP_EXACT))}


def main(argv):
    if "--record" not in argv:
        sys.exit(__doc__)
    if os.path.exists(GOLDEN) and "--force" not in argv:
        sys.exit(f"{GOLDEN} exists: pass --force to overwrite it")
    import gcm_amd
    gcm_amd.lib()
    out = run_all(gcm_amd)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(out)} runs from {gcm_amd.LIB_PATH} into {GOLDEN}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1:])
