#!/usr/bin/env python3
"""What a strided snapshot costs: every k-th node of an N^3 grid as Float32 arrays
on the host, against the whole box followed by numpy slicing, and the strided
pack kernel alone.  One JSON line.

    python scripts/bench_snapshot_strided.py --n 512 [--kernel-only] [--engine]
                                             [--out profiles/observe/strided_512.json]

borderSize 2, isotropic elastic, parity-random field, "Velocity" + PRESSURE.  One
process; host clock around synchronous calls, device events for the kernels
alone (gcmx_profile_*).  3 warm-ups, then 5 repetitions per variant, the variants
alternating.  The library is the package's, or the one GCMX_LIB names (a build
with another load rule along the contiguous axis: --label says which).

  arrays   strides (2,2,2) and (4,4,4).  box_then_slice: gcmx_snapshot_box in z
           slabs of at most --chunk-mib of output, then [::s] per axis into
           contiguous arrays -- all a user had before.  strided: one
           gcmx_snapshot_strided.  The results are compared bitwise.  Gate: strided
           faster in every one of the five alternating pairs.
  kernel   strides (2,2,2), (4,4,4), (1,1,2), (1,1,8): the strided k_pack_vtk alone
           on its line-granular traffic (per selected row and fp64 plane read
           min(128-byte lines of the row's span, output points of the row) lines,
           plus the Float32 written), alternating with the unit-stride kernel over
           the same box and with gcmx_copy_ceiling of the strided kernel's bytes.
  engine   (--engine) a run of --engine-steps steps at --engine-n^3 with a VTK
           snapshot every step: stride (4,4,4) against stride 1, wall ms per step
           including the files.

Exits 1 when the gate fails, 2 without a GPU."""
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
    ap.add_argument("--kernel-only", action="store_true", help="skip the host arrays")
    ap.add_argument("--engine", action="store_true", help="also the engine runs")
    ap.add_argument("--engine-n", type=int, default=256)
    ap.add_argument("--engine-steps", type=int, default=20)
    ap.add_argument("--label", default="", help="names the library build in the result")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_snapshot_strided: no GPU", file=sys.stderr)
        return 2
    import gcm_amd

    N, bs = a.n, 2
    sizes = [N, N, N]
    ctx = gcm_amd.Context(3, bs, sizes)
    ctx.fill_random(sizes, 0x5EED)
    ctx.sync()
    lib = gcm_amd.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    qcodes = (ctypes.c_int * 1)(PRESSURE)
    plane = N * N
    thick = max(1, (a.chunk_mib << 20) // (plane * 16))
    full_v = np.empty((N ** 3, 3), np.float32)
    full_q = np.empty(N ** 3, np.float32)

    def whole_box():
        for z0 in range(0, N, thick):
            z1 = min(N, z0 + thick)
            lo, hi = (ctypes.c_int * 3)(0, 0, z0), (ctypes.c_int * 3)(N, N, z1)
            first = z0 * plane
            st = lib.gcmx_snapshot_box(ctx.ptr, lo, hi, 1, 1, qcodes,
                                       ctypes.cast(full_v.ctypes.data + 12 * first, fp),
                                       ctypes.cast(full_q.ctypes.data + 4 * first, fp))
            if st != 0:
                raise RuntimeError(lib.gcmx_last_error().decode())

    def box_then_slice(s):
        whole_box()
        sl = tuple(slice(None, None, k) for k in s[::-1])
        return {"Velocity": np.ascontiguousarray(full_v.reshape(N, N, N, 3)[sl]).reshape(-1, 3),
                "pressure": np.ascontiguousarray(full_q.reshape(N, N, N)[sl]).reshape(-1)}

    def strided(s):
        vel, q = ctx.snapshot_strided([0, 0, 0], sizes, list(s), [PRESSURE])
        return {"Velocity": vel, "pressure": q[0]}

    res = {"bench": "snapshot_strided", "n": N, "border_size": bs, "chunk_mib": a.chunk_mib, "warmup": WARMUP,
           "reps": REPS, "label": a.label, "lib": os.environ.get("GCMX_LIB", "")}
    gate = True

    # ---- arrays on the host
    if not a.kernel_only:
        res["arrays"] = {}
        for s in ((2, 2, 2), (4, 4, 4)):
            variants = {"box_then_slice": box_then_slice, "strided": strided}
            times = {k: [] for k in variants}
            moved, last = {}, {}
            for rep in range(WARMUP + REPS):
                for name, fn in variants.items():
                    b0 = ctx.transfer_bytes()[0]
                    t0 = time.perf_counter()
                    last[name] = fn(s)
                    ms = (time.perf_counter() - t0) * 1e3
                    moved[name] = ctx.transfer_bytes()[0] - b0
                    if rep >= WARMUP:
                        times[name].append(ms)
                    say(f"  {'warm' if rep < WARMUP else 'rep '} {rep} {s} {name}: {ms:.1f} ms")
            for k in ("Velocity", "pressure"):
                x, y = last["box_then_slice"][k], last["strided"][k]
                if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                    print(f"bench_snapshot_strided: {k} differs between the two ways at {s}", file=sys.stderr)
                    return 1
            last.clear()
            pairs = [x / y for x, y in zip(times["box_then_slice"], times["strided"])]
            r = {k: dict(stats(v), bytes_to_host=int(moved[k])) for k, v in times.items()}
            r["pair_ratios"] = pairs
            r["ratio_of_medians"] = r["box_then_slice"]["median_ms"] / r["strided"]["median_ms"]
            r["byte_ratio"] = moved["box_then_slice"] / moved["strided"]
            r["faster_in_every_pair"] = bool(min(pairs) > 1.0)
            gate = gate and r["faster_in_every_pair"]
            res["arrays"]["x".join(map(str, s))] = r

    # ---- the kernels alone
    ctx.profile(True)
    res["kernel"] = {}
    for s in ((2, 2, 2), (4, 4, 4), (1, 1, 2), (1, 1, 8)):
        n_out = int(np.prod([-(-N // k) for k in s]))
        buf = np.empty(n_out * 4, np.float32)
        lo, hi, st = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(N, N, N), (ctypes.c_int * 3)(*s)

        def strided_call():
            if lib.gcmx_snapshot_strided(ctx.ptr, lo, hi, st, 1, 1, qcodes, ctypes.cast(buf.ctypes.data, fp),
                                         ctypes.cast(buf.ctypes.data + 12 * n_out, fp)) != 0:
                raise RuntimeError(lib.gcmx_last_error().decode())

        ms = {"strided": [], "unit": [], "ceiling": []}
        model_bytes = kernel = None
        for rep in range(WARMUP + REPS):
            ctx.profile_reset()
            strided_call()
            ctx.sync()
            pk = ctx.profile_read()["pack_vtk_strided"]
            model_bytes, kernel = pk["bytes_per_launch"], pk["kernel"]
            ctx.profile_reset()
            whole_box()
            ctx.sync()
            unit = ctx.profile_read()["pack_vtk"]["total_ms"]
            ceil = ctx.copy_ceiling_ms(int(model_bytes), 1)
            if rep >= WARMUP:
                ms["strided"].append(pk["total_ms"])
                ms["unit"].append(unit)
                ms["ceiling"].append(ceil)
        unit_bytes = N ** 3 * (6 * 8 + 16)
        r = {k: stats(v) for k, v in ms.items()}
        r.update(points=n_out, line_model_bytes=model_bytes, output_and_8_bytes=n_out * (6 * 8 + 16),
                 tbps=model_bytes / r["strided"]["median_ms"] / 1e9,
                 ratio_to_ceiling=r["ceiling"]["median_ms"] / r["strided"]["median_ms"],
                 unit_tbps=unit_bytes / r["unit"]["median_ms"] / 1e9,
                 unit_ratio_to_ceiling=(ctx.copy_ceiling_ms(unit_bytes, 3) / r["unit"]["median_ms"]))
        say(f"  kernel {s}: {r['strided']['median_ms']:.3f} ms, {r['tbps']:.2f} TB/s on the line model, "
            f"{r['ratio_to_ceiling']:.2f} of the copy ceiling; unit stride {r['unit']['median_ms']:.3f} ms "
            f"({r['unit_ratio_to_ceiling']:.2f} of its ceiling)")
        res["kernel"]["x".join(map(str, s))] = r
    ctx.close()

    # ---- the engine, a snapshot every step
    if a.engine:
        from gcm_amd import _gcm_host as H
        E, steps = a.engine_n, a.engine_steps

        def task(stride):
            t = H.Task()
            t.dimensionality = 3
            t.border_size = bs
            t.h = [1.0, 1.0, 1.0]
            t.courant = 0.9
            t.number_of_snaps = steps
            t.steps_per_snap = 1
            t.add_body(0, [E] * 3, [0, 0, 0])
            t.set_default_material(4.0, 2.0, 1.0)
            t.add_initial_quantity(("sphere", E / 8, (E / 2,) * 3), "PRESSURE", 10.0)
            t.add_snapshotter("VTK")
            t.set_vtk_quantities(["PRESSURE"])
            t.set_vtk_stride(list(stride))
            t.output_directory = "bench"
            return t

        eng = {}
        cwd = os.getcwd()
        for name, stride in (("stride_1", (1, 1, 1)), ("stride_4", (4, 4, 4))):
            with tempfile.TemporaryDirectory() as tmp:
                os.chdir(tmp)
                try:
                    he = H.Engine(task(stride))
                    t0 = time.perf_counter()
                    he.run()
                    he.sync(0)
                    ms = (time.perf_counter() - t0) * 1e3
                    eng[name] = {"steps": he.steps, "ms_per_step": ms / he.steps,
                                 "bytes_to_host": he.transfer_bytes(0)[0]}
                    say(f"  engine {name}: {ms / he.steps:.2f} ms per step over {he.steps} steps")
                finally:
                    os.chdir(cwd)
        res["engine"] = dict(eng, n=E)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main())
