#!/usr/bin/env python3
"""What a snapshot costs: the Float32 arrays of an N^3 grid ready on the host, the
whole-layer way against the device-packed way, and the pieces around it.  One
JSON line.

    python scripts/bench_snapshot.py --n 512 [--detector] [--out profiles/observe/snapshot_512.json]

borderSize 2, isotropic elastic, parity-random field, "Velocity" + PRESSURE (16
bytes per node in the file).  One process; host clock around synchronous calls
(every call below returns with its host buffers filled), device events for the
kernels alone (gcmx_profile_*).  3 warm-ups, then 5 repetitions per variant, the
variants alternating.

  arrays        layer_download: gcmx_download, then the GPU-free VtkSnapshotter array
                loop over the layer (vtk_layer_arrays) -- what a snapshot did before.
                snapshot_box: gcmx_snapshot_box in z slabs of at most --chunk-mib of
                output, written straight into the file's arrays -- what
                VtkSnapshotter does now.  Gate: snapshot_box at least 3x faster.
                The two results are compared bitwise before anything is printed.
  pack_vtk      k_pack_vtk alone (events) on its algorithmic bytes, 6 fp64 planes read
                + 16 B written per node, against gcmx_copy_ceiling of the same bytes.
  scan          gcmx_scan: ms per call, the kernel alone, fraction of 8 TB/s on the
                inner 72 B per node.
  detector      (--detector, an engine run of about 50 steps at N^3): SLICESNAP at
                stepsPerSnap = 1 against no snapshotter, ms per step; and the layer
                download (HipMesh::pdeAll) the snapshotter made per step before,
                timed on two calls.

Exits 1 when the 3x gate fails, 2 without a GPU."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, REPS = 3, 5
PRESSURE = 12


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True, help="grid size (N^3 nodes)")
    ap.add_argument("--chunk-mib", type=int, default=256, help="output bytes per snapshot_box call")
    ap.add_argument("--detector", action="store_true", help="also the 50-step engine runs")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_snapshot: no GPU", file=sys.stderr)
        return 2
    import gcm_amd
    from gcm_amd import _gcm_host as H

    N, bs = a.n, 2
    sizes = [N, N, N]
    n = N ** 3
    ctx = gcm_amd.Context(3, bs, sizes)
    ctx.fill_random(sizes, 0x5EED)
    ctx.sync()
    lib = gcm_amd.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    qcodes = (ctypes.c_int * 1)(PRESSURE)
    plane = N * N
    thick = max(1, (a.chunk_mib << 20) // (plane * 16))

    def layer_download():
        pde = ctx.download()
        return H.vtk_layer_arrays(sizes, bs, pde, ["PRESSURE"])

    def snapshot_box():
        vel = np.empty((n, 3), np.float32)
        q = np.empty(n, np.float32)
        for z0 in range(0, N, thick):
            z1 = min(N, z0 + thick)
            lo, hi = (ctypes.c_int * 3)(0, 0, z0), (ctypes.c_int * 3)(N, N, z1)
            first = z0 * plane
            st = lib.gcmx_snapshot_box(ctx.ptr, lo, hi, 1, 1, qcodes,
                                       ctypes.cast(vel.ctypes.data + 12 * first, fp),
                                       ctypes.cast(q.ctypes.data + 4 * first, fp))
            if st != 0:
                raise RuntimeError(lib.gcmx_last_error().decode())
        return {"Velocity": vel, "pressure": q}

    variants = {"layer_download": layer_download, "snapshot_box": snapshot_box}
    times = {k: [] for k in variants}
    moved = {}
    last = {}
    for rep in range(WARMUP + REPS):
        for name, fn in variants.items():
            b0 = ctx.transfer_bytes()[0]
            t0 = time.perf_counter()
            last[name] = fn()
            ms = (time.perf_counter() - t0) * 1e3
            moved[name] = ctx.transfer_bytes()[0] - b0
            if rep >= WARMUP:
                times[name].append(ms)
            say(f"  {'warm' if rep < WARMUP else 'rep '} {rep} {name}: {ms:.1f} ms")
    for k in ("Velocity", "pressure"):
        x, y = last["layer_download"][k], last["snapshot_box"][k]
        if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            print(f"bench_snapshot: {k} differs between the two ways", file=sys.stderr)
            return 1
    last.clear()
    arrays = {k: dict(stats(v), bytes_to_host=int(moved[k])) for k, v in times.items()}
    speedup = arrays["layer_download"]["median_ms"] / arrays["snapshot_box"]["median_ms"]
    arrays["speedup"] = speedup
    arrays["byte_ratio"] = moved["layer_download"] / moved["snapshot_box"]
    arrays["gate_3x"] = bool(speedup >= 3.0)

    # ---- k_pack_vtk alone
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(REPS):
        snapshot_box()
    ctx.sync()
    pk = ctx.profile_read()["pack_vtk"]
    launches_per_box = -(-N // thick)
    pack_ms = pk["total_ms"] / REPS
    pack_bytes = n * (6 * 8 + 16)
    assert abs(pk["bytes_per_launch"] * launches_per_box - pack_bytes) <= 1e-6 * pack_bytes, pk
    ceiling_ms = ctx.copy_ceiling_ms(pack_bytes, 5)
    pack = {"ms_per_box": pack_ms, "launches_per_box": launches_per_box, "algorithmic_bytes": pack_bytes,
            "tbps": pack_bytes / pack_ms / 1e9, "copy_ceiling_ms": ceiling_ms,
            "copy_ceiling_tbps": pack_bytes / ceiling_ms / 1e9, "ratio_to_ceiling": ceiling_ms / pack_ms,
            "kernel": pk["kernel"]}

    # ---- gcmx_scan
    ctx.profile_reset()
    scan_ms = []
    for rep in range(WARMUP + REPS):
        t0 = time.perf_counter()
        bad, mx = ctx.scan()
        if rep >= WARMUP:
            scan_ms.append((time.perf_counter() - t0) * 1e3)
    sk = ctx.profile_read()["scan"]
    kernel_ms = sk["total_ms"] / sk["launches"]
    scan = dict(stats(scan_ms), kernel_ms=kernel_ms, nonfinite=bad, max_abs=float(mx.max()),
                fraction_of_8tbps=n * 72 / (kernel_ms * 1e-3) / 8e12)
    ctx.close()

    res = {"bench": "snapshot", "n": N, "border_size": bs, "chunk_mib": a.chunk_mib, "warmup": WARMUP,
           "reps": REPS, "arrays": arrays, "pack_vtk": pack, "scan": scan}

    # ---- detector every step
    if a.detector:
        def task(slicesnap):
            t = H.Task()
            t.dimensionality = 3
            t.border_size = bs
            t.h = [1.0, 1.0, 1.0]
            t.courant = 0.9
            t.number_of_snaps = 50
            t.steps_per_snap = 1
            t.add_body(0, sizes, [0, 0, 0])
            t.set_default_material(4.0, 2.0, 1.0)
            t.add_initial_quantity(("sphere", N / 8, (N / 2,) * 3), "PRESSURE", 10.0)
            if slicesnap:
                t.add_snapshotter("SLICESNAP")
                t.set_detector(["Szz"], ("box", (-1, -1, -1), (2.0 * N,) * 3), 0)
                t.output_directory = "bench"
            return t

        det = {}
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                for name, on in (("no_snapshotter", False), ("slicesnap_every_step", True)):
                    he = H.Engine(task(on))
                    he.run_steps(3)
                    he.sync(0)
                    he = H.Engine(task(on))
                    t0 = time.perf_counter()
                    he.run()
                    he.sync(0)
                    ms = (time.perf_counter() - t0) * 1e3
                    # requiredTime is 50 time steps' worth; the accumulated clock may take one more
                    det[name] = {"steps": he.steps, "ms_per_step": ms / he.steps,
                                 "bytes_to_host": he.transfer_bytes(0)[0]}
                    say(f"  engine {name}: {ms / he.steps:.3f} ms per step over {he.steps} steps")
                    if on:
                        dl = []
                        for _ in range(2):
                            t0 = time.perf_counter()
                            he.pde(0)
                            dl.append((time.perf_counter() - t0) * 1e3)
                        det["layer_download_per_snapshot_before_ms"] = dl
            finally:
                os.chdir(cwd)
        res["detector"] = det

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if arrays["gate_3x"] else 1


if __name__ == "__main__":
    sys.exit(main())
