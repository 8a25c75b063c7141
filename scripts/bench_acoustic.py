#!/usr/bin/env python3
"""Step time of the one-pass acoustic step (k_step_acoustic) on an N^3 grid of
one GPU, against the generic per-stage kernel on the same matrices and the
isotropic elastic default step.  One JSON line.

    python scripts/bench_acoustic.py --n 512 [--bs 2] [--out profiles/acoustic/bench_512.json]

Material: rho 2, lambda 8 (c = 2), h = 1, parity-random field (fill_random).
Variants, all in one process, 3 warm-up steps each, then 5 windows of >= 20
steps per variant timed with device events on the context's stream, the
variants alternating:

    acoustic          acoustic context, path AUTO, Courant 0.9 (the KF0 instance)
    acoustic_courant1 the same at Courant 1: every foot on a node (q = 1, the
                      !KF0 instance), the natural acoustic setting
    acoustic_generic  the same matrices under GCMX_PATH_GENERIC at Courant 0.9
                      (k_stage_generic x 3)
    iso_default       isotropic elastic (4, 2, 1), the default step, for context

Per variant: median / min / max ms per step, Mnode-steps/s and the fraction of
8 TB/s on the variant's bytes per node-step (64 B acoustic, 144 B elastic: a
one-pass step moves each layer once).  Before printing, the final states of
`acoustic` and `acoustic_generic` are compared bitwise.  The two gates of the
acoustic step are reported and decide the exit status: at 512^3 `acoustic` is
not slower than `iso_default`; at every size it is faster than
`acoustic_generic`.  Exits non-zero without a GPU or when a check fails."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RHO, LAM = 2.0, 8.0
WARMUP, WINDOWS = 3, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True, help="grid size (N^3 nodes)")
    ap.add_argument("--bs", type=int, default=2, help="borderSize (ghost depth)")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window (>= 20)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    steps = max(20, a.steps)
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_acoustic: no GPU", file=sys.stderr)
        return 2
    import gcm_amd
    from gcm_amd.host import acoustic_matrices, isotropic_elastic_matrices

    N, bs = a.n, a.bs
    aU, aU1, aL = acoustic_matrices(3, RHO, LAM)
    iU, iU1, iL = isotropic_elastic_matrices(3, 4.0, 2.0, 1.0)
    c_ac = float(np.max(np.abs(aL)))
    tau_a = 0.9 * 1.0 / c_ac
    tau_1 = 1.0 * 1.0 / c_ac
    tau_i = 0.9 * 1.0 / float(np.max(np.abs(iL)))

    def make(U, U1, L, model, path):
        c = gcm_amd.Context(3, bs, [N, N, N], device=0, model=model)
        c.set_materials(U[None], U1[None], L[None])
        if path is not None:
            c.set_path(path)
        c.fill_random([N, N, N], 0x5EED)
        return c

    variants = [("acoustic", make(aU, aU1, aL, "acoustic", None), tau_a, 64),
                ("acoustic_courant1", make(aU, aU1, aL, "acoustic", None), tau_1, 64),
                ("acoustic_generic", make(aU, aU1, aL, "acoustic", gcm_amd.PATH_GENERIC), tau_a, 64),
                ("iso_default", make(iU, iU1, iL, "elastic", None), tau_i, 144)]
    kernels, times = {}, {v[0]: [] for v in variants}
    for name, c, tau, _ in variants:
        c.profile(True)
        for _ in range(WARMUP):
            c.step(tau)
        c.sync()
        kernels[name] = sorted({v["kernel"] for v in c.profile_read().values() if v["launches"] > 0})
        c.profile(False)
    for _ in range(WINDOWS):
        for name, c, tau, _ in variants:
            st = torch.cuda.ExternalStream(c.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(steps):
                c.step(tau)
            e1.record(st)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)

    # the two compared variants have run the same steps from the same field
    ctx = {v[0]: v[1] for v in variants}
    one = ctx["acoustic"].download()
    same = bool(np.array_equal(one, ctx["acoustic_generic"].download()))
    finite = bool(np.isfinite(one).all())
    del one

    nodes = float(N) ** 3
    out = {"n": N, "bs": bs, "steps_per_window": steps, "windows": WINDOWS, "warmup_steps": WARMUP,
           "bound": "HBM", "peak_tb_s": 8.0, "variants": {}}
    for name, c, _, node_bytes in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        out["variants"][name] = {"median_ms": round(med, 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                                 "mnode_steps_per_s": round(nodes / (med * 1e-3) / 1e6, 1),
                                 "bytes_per_node_step": node_bytes,
                                 "hbm_frac": round(node_bytes * nodes / (med * 1e-3) / 8e12, 4),
                                 "path": c.last_path, "kernels": kernels[name]}
    v = out["variants"]
    out["generic_over_acoustic"] = round(v["acoustic_generic"]["median_ms"] / v["acoustic"]["median_ms"], 3)
    out["iso_default_over_acoustic"] = round(v["iso_default"]["median_ms"] / v["acoustic"]["median_ms"], 3)
    gate1 = v["acoustic"]["median_ms"] <= v["iso_default"]["median_ms"]
    gate2 = v["acoustic"]["median_ms"] < v["acoustic_generic"]["median_ms"]
    out["gates"] = {"not_slower_than_iso_default": bool(gate1), "faster_than_generic_stages": bool(gate2)}
    out["check"] = {"acoustic_equals_generic_bitwise": same, "finite": finite, "steps_each": WARMUP + WINDOWS * steps}
    for _, c, _, _ in variants:
        c.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same and finite and gate2 and (gate1 or N < 512) else 1


if __name__ == "__main__":
    sys.exit(main())
