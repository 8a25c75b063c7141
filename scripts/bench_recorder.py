#!/usr/bin/env python3
"""What a seismogram costs per step: 4096 random node receivers, two quantities,
recorded every step of a run.  One JSON line, also written to --out.

    python scripts/bench_recorder.py [--out profiles/recorder/bench.json]

Two grids, isotropic elastic, borderSize 2, parity-random field: 256^3 and a 2-D
2048^2.  One process; 3 warm-up steps per variant, then five windows of 200
steps per variant, the variants alternating; a window is timed with device
events on the context's stream and with the host clock (the stream drained at
its end).
  steps    gcmx_step only
  gather   gcmx_step, then gcmx_gather: the only way before the recorder -- a wait
           for the stream and a copy to the host every step
  record   gcmx_step, then gcmx_record; one gcmx_recorder_read (and reset) every
           256 steps, wherever in a window that falls
The result holds ms per step per variant and window, and per window pair the
cost over `steps` of `gather` and of `record`.  No ratio is a gate: the script
reports.  Exits 2 without a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, WINDOWS, STEPS, RECEIVERS, BATCH = 3, 5, 200, 4096, 256


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def bench_grid(gcm_amd, torch, sizes):
    from gcm_amd.host import isotropic_elastic_matrices
    D = len(sizes)
    lib = gcm_amd.lib()
    ctx = gcm_amd.Context(D, 2, sizes)
    U, U1, L = isotropic_elastic_matrices(D, 4.0, 2.0, 1.0)
    ctx.set_materials(U[None], U1[None], L[None])
    ctx.fill_random(sizes, 0x5EED)
    tau = 0.9
    rng = np.random.default_rng(4096)
    nodes = np.stack([rng.integers(0, s, RECEIVERS) for s in sizes], axis=1).astype(np.int32)
    codes = [2 + D - 1, 12]
    nl = ctx.node_list(nodes)
    rec = ctx.recorder(nl, codes, BATCH)
    qs = (ctypes.c_int * 2)(*codes)
    dp = ctypes.POINTER(ctypes.c_double)
    one = np.empty((2, RECEIVERS))
    batch = np.empty((BATCH, 2, RECEIVERS))
    stream = torch.cuda.ExternalStream(ctx.stream)

    def ok(status):
        if status != 0:
            raise RuntimeError(lib.gcmx_last_error().decode())

    def steps_only():
        ok(lib.gcmx_step(ctx.ptr, tau))

    def gather():
        ok(lib.gcmx_step(ctx.ptr, tau))
        ok(lib.gcmx_gather(ctx.ptr, nl.ptr, 2, qs, one.ctypes.data_as(dp)))

    def record():
        ok(lib.gcmx_step(ctx.ptr, tau))
        ok(lib.gcmx_record(ctx.ptr, rec.ptr))
        if lib.gcmx_recorder_count(rec.ptr) == BATCH:
            ok(lib.gcmx_recorder_read(rec.ptr, 0, BATCH, batch.ctypes.data_as(dp)))
            ok(lib.gcmx_recorder_reset(rec.ptr))

    variants = {"steps": steps_only, "gather": gather, "record": record}
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    ctx.sync()
    out = {k: {"device_ms_per_step": [], "wall_ms_per_step": []} for k in variants}
    for w in range(WINDOWS):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(STEPS):
                fn()
            e1.record(stream)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3 / STEPS
            dev = e0.elapsed_time(e1) / STEPS
            out[name]["device_ms_per_step"].append(dev)
            out[name]["wall_ms_per_step"].append(wall)
            say(f"  {sizes} window {w} {name}: {dev:.4f} ms/step on the device, {wall:.4f} wall")
    for clock in ("device", "wall"):
        key = clock + "_ms_per_step"
        base = out["steps"][key]
        g = [x - b for x, b in zip(out["gather"][key], base)]
        r = [x - b for x, b in zip(out["record"][key], base)]
        out[clock + "_cost_over_steps"] = {"gather": g, "record": r,
                                           "record_below_gather_in_every_window": bool(all(x < y for x, y in zip(r, g)))}
    out["steps_recorded"] = (WARMUP + WINDOWS * STEPS)
    rec.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/recorder/bench.json")
    a = ap.parse_args()
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_recorder: no GPU", file=sys.stderr)
        return 2
    import gcm_amd
    res = {"bench": "recorder", "border_size": 2, "receivers": RECEIVERS, "quantities": 2, "warmup_steps": WARMUP,
           "windows": WINDOWS, "steps_per_window": STEPS, "read_every": BATCH,
           "device": torch.cuda.get_device_name(0)}
    res["256x256x256"] = bench_grid(gcm_amd, torch, [256, 256, 256])
    res["2048x2048"] = bench_grid(gcm_amd, torch, [2048, 2048])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
