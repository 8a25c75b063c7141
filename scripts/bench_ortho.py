#!/usr/bin/env python3
"""Step time of the one-pass orthotropic step (k_step_ortho) on an N^3 grid of
one GPU, against the generic per-stage kernels on the same matrices and the
isotropic default step.  One JSON line.

    python scripts/bench_ortho.py --n 512 [--bs 2] [--materials K --layout layers|random]

Material: rho 4, c = {360, 70, 60, 180, 50, 90, 10, 20, 30} (nine distinct
speeds), h = 1, Courant 0.9, parity-random field (fill_random).  Variants, all
in one process, 3 warm-up steps each, then 5 windows of >= 20 steps per variant
timed with device events on the context's stream, the variants alternating:

    ortho_fma      orthotropic, path AUTO, GCMX_FP_FMA (the product default)
    ortho_exact    orthotropic, path AUTO, GCMX_FP_EXACT
    ortho_generic  the same matrices under GCMX_PATH_GENERIC (k_stage_generic x 3,
                   what these matrices ran before the one-pass step existed)
    iso_default    isotropic (4, 2, 1), the default step, for context

Per variant: median / min / max ms per step, Mnode-steps/s and the fraction of
8 TB/s on 144 B per node-step (the one pass is HBM-bound: it moves each layer
once).  Before printing, the final states are compared: ortho_exact ==
ortho_generic bitwise, ortho_fma within 1e-10 relative L2 of ortho_exact.
Exits non-zero without a GPU or when that check fails.

--materials K > 1 measures per-node materials instead (k_step_ortho<..., HET>):
material k is the one above with its constants scaled by 1 + 0.05 k, odd k also
turned by 90 degrees about z (gcm_amd.host.cross_ply, the other ply of a
cross-ply laminate); --layout layers gives K equal slabs along y, random gives
uniformly random ids; tau is Courant 0.9 on the fastest material.  Variants:

    het_fma      per-node materials, path AUTO, GCMX_FP_FMA
    het_exact    per-node materials, path AUTO, GCMX_FP_EXACT
    het_generic  the same matrices and ids under GCMX_PATH_GENERIC (what they
                 ran before the heterogeneous one-pass step existed)
    ortho_fma    material 0 alone on the homogeneous one-pass step, for context

with 145 B per node-step (one id byte) and the same end-of-run checks:
het_exact == het_generic bitwise, het_fma within 1e-10 of het_exact."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MAT_A = (4.0, (360.0, 70.0, 60.0, 180.0, 50.0, 90.0, 10.0, 20.0, 30.0))
WARMUP, WINDOWS = 3, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True, help="grid size (N^3 nodes)")
    ap.add_argument("--bs", type=int, default=2, help="borderSize (ghost depth)")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window (>= 20)")
    ap.add_argument("--materials", type=int, default=1, help="materials (1: the homogeneous step)")
    ap.add_argument("--layout", choices=("layers", "random"), default="layers", help="per-node ids for --materials > 1")
    a = ap.parse_args()
    steps = max(20, a.steps)
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_ortho: no GPU", file=sys.stderr)
        return 2
    import gcm_amd
    from gcm_amd.host import cross_ply, isotropic_elastic_matrices, orthotropic_elastic_matrices

    N, bs, K = a.n, a.bs, a.materials
    if not 1 <= K <= 255:
        ap.error("--materials must be 1..255")
    oU, oU1, oL = orthotropic_elastic_matrices(*MAT_A)
    iU, iU1, iL = isotropic_elastic_matrices(3, 4.0, 2.0, 1.0)
    tau_o = 0.9 * 1.0 / float(np.max(np.abs(oL)))
    tau_i = 0.9 * 1.0 / float(np.max(np.abs(iL)))

    def make(U, U1, L, fp, path, ids=None):
        c = gcm_amd.Context(3, bs, [N, N, N], device=0)
        if ids is None:
            c.set_materials(U[None], U1[None], L[None])
        else:
            c.set_materials(U, U1, L)
            c.set_material_ids(ids)
        c.fp_mode = fp
        if path is not None:
            c.set_path(path)
        c.fill_random([N, N, N], 0x5EED)
        return c

    if K == 1:
        fast, exact_name, generic_name, node_bytes = "ortho_fma", "ortho_exact", "ortho_generic", 144
        variants = [("ortho_fma", make(oU, oU1, oL, gcm_amd.FP_FMA, None), tau_o),
                    ("ortho_exact", make(oU, oU1, oL, gcm_amd.FP_EXACT, None), tau_o),
                    ("ortho_generic", make(oU, oU1, oL, gcm_amd.FP_EXACT, gcm_amd.PATH_GENERIC), tau_o),
                    ("iso_default", make(iU, iU1, iL, gcm_amd.FP_FMA, None), tau_i)]
    else:
        fast, exact_name, generic_name, node_bytes = "het_fma", "het_exact", "het_generic", 145
        mats = []
        for k in range(K):
            c = tuple(v * (1 + 0.05 * k) for v in MAT_A[1])
            mats.append(orthotropic_elastic_matrices(MAT_A[0], cross_ply(c) if k % 2 else c))
        hU, hU1, hL = (np.stack([m[i] for m in mats]) for i in range(3))
        tau_h = 0.9 * 1.0 / float(np.max(np.abs(hL)))
        ids = np.zeros((N + 2 * bs,) * 3, dtype=np.uint8)  # all nodes, ghosts keep 0
        if a.layout == "layers":
            ids[bs:-bs, bs:-bs, bs:-bs] = (np.arange(N) * K // N).astype(np.uint8)[None, :, None]
        else:
            ids[bs:-bs, bs:-bs, bs:-bs] = np.random.default_rng(0x5EED).integers(0, K, (N, N, N), dtype=np.uint8)
        variants = [("het_fma", make(hU, hU1, hL, gcm_amd.FP_FMA, None, ids), tau_h),
                    ("het_exact", make(hU, hU1, hL, gcm_amd.FP_EXACT, None, ids), tau_h),
                    ("het_generic", make(hU, hU1, hL, gcm_amd.FP_EXACT, gcm_amd.PATH_GENERIC, ids), tau_h),
                    ("ortho_fma", make(oU, oU1, oL, gcm_amd.FP_FMA, None), tau_h)]
        del ids
    kernels, times = {}, {name: [] for name, _, _ in variants}
    for name, c, tau in variants:
        c.profile(True)
        for _ in range(WARMUP):
            c.step(tau)
        c.sync()
        kernels[name] = sorted({v["kernel"] for v in c.profile_read().values() if v["launches"] > 0})
        c.profile(False)
    for _ in range(WINDOWS):
        for name, c, tau in variants:
            st = torch.cuda.ExternalStream(c.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(steps):
                c.step(tau)
            e1.record(st)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)

    # the three compared variants have run the same steps from the same field
    ctx = {name: c for name, c, _ in variants}
    exact = ctx[exact_name].download()
    generic = ctx[generic_name].download()
    same = bool(np.array_equal(exact, generic))
    del generic
    fma = ctx[fast].download()
    fma -= exact
    rel = float(np.linalg.norm(fma.reshape(-1)) / np.linalg.norm(exact.reshape(-1)))
    del fma, exact

    nodes = float(N) ** 3
    out = {"n": N, "bs": bs, "steps_per_window": steps, "windows": WINDOWS, "warmup_steps": WARMUP,
           "bytes_per_node_step": node_bytes, "bound": "HBM", "peak_tb_s": 8.0, "variants": {}}
    if K > 1:
        out["materials"], out["layout"] = K, a.layout
    for name, c, _ in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        out["variants"][name] = {"median_ms": round(med, 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                                 "mnode_steps_per_s": round(nodes / (med * 1e-3) / 1e6, 1),
                                 "hbm_frac_144B": round(144 * nodes / (med * 1e-3) / 8e12, 4),
                                 "path": c.last_path, "kernels": kernels[name]}
    v = out["variants"]
    out["generic_over_fma"] = round(v[generic_name]["median_ms"] / v[fast]["median_ms"], 3)
    out["generic_over_exact"] = round(v[generic_name]["median_ms"] / v[exact_name]["median_ms"], 3)
    if K > 1:
        out["het_fma_over_ortho_fma"] = round(v["het_fma"]["median_ms"] / v["ortho_fma"]["median_ms"], 3)
    out["check"] = {"exact_equals_generic_bitwise": same, "fma_vs_exact_rel_l2": rel,
                    "steps_each": WARMUP + WINDOWS * steps}
    for _, c, _ in variants:
        c.close()
    print(json.dumps(out), flush=True)
    return 0 if same and rel <= 1e-10 else 1


if __name__ == "__main__":
    sys.exit(main())
