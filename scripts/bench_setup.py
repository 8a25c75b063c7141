#!/usr/bin/env python3
"""What setting a body up costs: materials and initial state by areas, formed on
the device (gcmx_setup_*, Task.set_device_setup(True)) against the host loops and
the layer upload (buildHostState + gcmx_set_material_ids + gcmx_upload).  One
JSON line.

    python scripts/bench_setup.py --n 256 [--no-baseline] [--out profiles/setup/setup_256.json]

N^3 nodes, borderSize 2, isotropic elastic, a set-up of the size the reference's
tasks use: the default material plus two areas (a slab and a spherical
inclusion), one PRESSURE quantity in a sphere plus one P wave in a slab.  One
process, 3 warm-ups, 5 timed repetitions, device events.

  kernel    k_setup_state alone (gcmx_profile_*, events around the launch) on the
            72 bytes per inner node it writes, alternating with the ceiling: a
            torch zero_() of the same number of bytes (events on torch's stream).
            fraction_of_fill = fill time / kernel time.  k_setup_ids (one byte per
            node) and the census (no store) are timed the same way.
  engine    wall time of Engine(task) with the flag on; and, unless --no-baseline,
            with it off -- the path before -- with both byte counts of
            gcmx_transfer_stats; at --check sizes the two layers are compared
            bitwise (a download each)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, REPS = 3, 5


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True, help="grid size (N^3 nodes)")
    ap.add_argument("--no-baseline", action="store_true", help="skip the host path (it needs 2 x 72 B per node of host memory)")
    ap.add_argument("--check", action="store_true", help="compare the two engines' layers bitwise")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_setup: no GPU", file=sys.stderr)
        return 2
    import gcm_amd
    from gcm_amd import _gcm_host as H
    from oracle import oracle as O

    N, bs = a.n, 2
    sizes = [N, N, N]
    n = N ** 3
    slab = ("box", (-1.0, -1.0, 0.6 * N), (2.0 * N, 2.0 * N, 0.8 * N))
    inclusion = ("sphere", N / 6.0, (0.3 * N, 0.4 * N, 0.35 * N))
    source = ("sphere", N / 8.0, (N / 2.0,) * 3)
    front = ("box", (-1.0, -1.0, 0.1 * N), (2.0 * N, 2.0 * N, 0.2 * N))
    materials = [(4.0, 2.0, 1.0), (2.0, 1.0, 1.0), (8.0, 4.0, 2.0)]

    # ---- the kernels alone, on a context
    U, U1, L = (np.stack(x) for x in zip(*[O.isotropic_elastic_matrices(3, *m) for m in materials]))
    pressure = np.zeros(9)
    O.quantity_set(3, "PRESSURE", 10.0, pressure)
    wave = U1[0][2][:, O.WAVE_COLUMN["P_FORWARD"]].copy()
    wave = wave * (-2.0 / float(O.quantity_get(3, "Vz", wave)))
    ctx = gcm_amd.Context(3, bs, sizes)
    ctx.set_materials(U, U1, L)
    ctx.profile(True)
    fill = torch.empty(n * 9, dtype=torch.float64, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    mat_areas = [("infinite",), slab, inclusion]

    def timed(name, call):
        ctx.profile_reset()
        call()
        ctx.sync()
        b = ctx.profile_read()[name]
        assert b["launches"] == 1, b
        return b["total_ms"]

    k_ms = {"setup_state": [], "setup_ids": [], "setup_census": [], "fill": []}
    for rep in range(WARMUP + REPS):
        ms = {"setup_state": timed("setup_state", lambda: ctx.setup_state([source, front], [pressure, wave])),
              "setup_census": timed("setup_census", lambda: ctx.setup_census(mat_areas, [0, 1, 2])),
              "setup_ids": timed("setup_ids", lambda: ctx.setup_material_ids(mat_areas, [0, 1, 2]))}
        ev0.record()
        fill.zero_()
        ev1.record()
        torch.cuda.synchronize()
        ms["fill"] = ev0.elapsed_time(ev1)
        say(f"  {'warm' if rep < WARMUP else 'rep '} {rep}: " + ", ".join(f"{k} {v:.3f} ms" for k, v in ms.items()))
        if rep >= WARMUP:
            for k, v in ms.items():
                k_ms[k].append(v)
    kernel = {k: stats(v) for k, v in k_ms.items()}
    state_bytes = n * 72
    kernel["state_bytes"] = state_bytes
    kernel["setup_state_tbps"] = state_bytes / kernel["setup_state"]["median_ms"] / 1e9
    kernel["fill_tbps"] = state_bytes / kernel["fill"]["median_ms"] / 1e9
    kernel["fraction_of_fill"] = kernel["fill"]["median_ms"] / kernel["setup_state"]["median_ms"]
    used = [int(v) for v in ctx.setup_census(mat_areas, [0, 1, 2])]
    ctx.close()
    del fill

    # ---- the engine's set-up, wall time
    def task(flag):
        t = H.Task()
        t.dimensionality = 3
        t.border_size = bs
        t.h = [1.0, 1.0, 1.0]
        t.courant = 0.9
        t.number_of_snaps = 1
        t.add_body(0, sizes, [0, 0, 0])
        t.set_default_material(*materials[0])
        t.add_material(slab, *materials[1])
        t.add_material(inclusion, *materials[2])
        t.add_initial_quantity(source, "PRESSURE", 10.0)
        t.add_initial_wave(front, "P_FORWARD", 2, "Vz", -2.0)
        t.set_device_setup(flag)
        return t

    engine = {}
    layers = {}
    for name, flag in (("device", True),) + ((() if a.no_baseline else (("host", False),))):
        reps = REPS if flag else 1  # the host path takes seconds to minutes: once
        ms = []
        for rep in range((WARMUP if flag else 0) + reps):
            t0 = time.perf_counter()
            e = H.Engine(task(flag))
            e.sync(0)
            dt = (time.perf_counter() - t0) * 1e3
            say(f"  engine set-up, {name}: {dt:.1f} ms")
            if rep >= (WARMUP if flag else 0):
                ms.append(dt)
            d2h, h2d = e.transfer_bytes(0)
            path = e.path(0)
            if a.check and rep == 0:
                layers[name] = e.pde(0)
            del e
        engine[name] = dict(stats(ms), reps=len(ms), bytes_to_device=int(h2d), bytes_to_host=int(d2h), path=path)
    if "host" in engine:
        engine["speedup"] = engine["host"]["median_ms"] / engine["device"]["median_ms"]
        engine["byte_ratio"] = engine["host"]["bytes_to_device"] / max(1, engine["device"]["bytes_to_device"])
    if len(layers) == 2:
        engine["layers_equal_bitwise"] = bool(np.array_equal(layers["host"].view(np.uint64), layers["device"].view(np.uint64)))
    layers.clear()

    res = {"bench": "setup", "n": N, "border_size": bs, "warmup": WARMUP, "reps": REPS, "materials_used": used,
           "kernel": kernel, "engine": engine}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if engine.get("layers_equal_bitwise", True) else 1


if __name__ == "__main__":
    sys.exit(main())
