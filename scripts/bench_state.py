#!/usr/bin/env python3
"""What the exact state costs on its way out of the device and back: the box calls
(gcmx_read_box / gcmx_write_box of every inner node) against the whole-layer calls
(gcmx_download / gcmx_upload), every one into or from a preallocated host array;
the two state kernels alone against a flat copy of the same bytes; and, with
--engine, one save_state and one load_state of an engine.  One JSON line.

    python scripts/bench_state.py --n 512 [--out profiles/state/state_512.json]
    python scripts/bench_state.py --n 1024 --engine-only [--dir /some/disk] [--out ...]

borderSize 2, isotropic elastic (M = 9), parity-random field.  One process; host
clock around synchronous calls, device events for the kernels alone
(gcmx_profile_*).  3 warm-ups, then 5 repetitions per variant, the variants
alternating.

  rss           before anything whole-layer runs: one read_box and one write_box of
                the inner nodes with the caller's one array.  The peak resident set
                may grow by that array and a small allowance (5 % + 256 MiB), or the
                library allocated something the size of the box.
  calls         download / read_box / upload / write_box in turn.  Gate: the box call
                is faster than the layer call in every one of the five pairs, in both
                directions.  read_box's array is compared bitwise with download's
                inner nodes, and the layer after write_box with the layer before.
  kernels       k_state_pack<9> and k_state_unpack<9> alone (events around the chunk
                launches, summed per box: 144 B per node) against gcmx_copy_ceiling
                of the same bytes, alternating.  A record, not a gate.
  engine        (--engine / --engine-only) a device-set-up N^3 engine: one step, then
                save_state and load_state once each, seconds and file size; skipped
                with the reason when the disk lacks the room.

Exits 1 when a gate fails, 2 without a GPU."""
import argparse
import ctypes
import json
import os
import resource
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, REPS = 3, 5
M = 9


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "all_ms": [round(x, 2) for x in ms]}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def rss_now():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def rss_peak():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def calls_and_kernels(a, gcm_amd):
    N, bs = a.n, 2
    sizes = [N, N, N]
    n = N ** 3
    ctx = gcm_amd.Context(3, bs, sizes)
    ctx.fill_random(sizes, 0x5EED)
    ctx.sync()
    lib = gcm_amd.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    lo, hi = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(N, N, N)
    stage = a.stage_mib << 20

    def check(st):
        if st != 0:
            raise RuntimeError(lib.gcmx_last_error().decode())

    # ---- the box calls alone: what the process's memory grows by
    rss0 = rss_now()
    box = np.empty((N, N, N, M))
    box_p = box.ctypes.data_as(dp)
    check(lib.gcmx_read_box(ctx.ptr, lo, hi, box_p, stage))
    check(lib.gcmx_write_box(ctx.ptr, lo, hi, box_p, stage))
    grown = rss_peak() - rss0
    allowed = int(box.nbytes * 1.05) + (256 << 20)
    rss = {"before_bytes": rss0, "peak_growth_bytes": grown, "caller_array_bytes": box.nbytes,
           "allowed_growth_bytes": allowed, "gate_no_box_sized_allocation": bool(grown <= allowed)}
    say(f"  rss: grew {grown / 2**30:.2f} GiB for a caller's array of {box.nbytes / 2**30:.2f} GiB")

    # ---- the calls, alternating
    layer = np.empty((N + 2 * bs,) * 3 + (M,))
    layer_p = layer.ctypes.data_as(dp)
    variants = {"download": lambda: check(lib.gcmx_download(ctx.ptr, layer_p)),
                "read_box": lambda: check(lib.gcmx_read_box(ctx.ptr, lo, hi, box_p, stage)),
                "upload": lambda: check(lib.gcmx_upload(ctx.ptr, layer_p)),
                "write_box": lambda: check(lib.gcmx_write_box(ctx.ptr, lo, hi, box_p, stage))}
    times = {k: [] for k in variants}
    moved = {}
    for rep in range(WARMUP + REPS):
        for name, fn in variants.items():
            b0 = ctx.transfer_bytes()
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            b1 = ctx.transfer_bytes()
            moved[name] = (b1[0] - b0[0]) + (b1[1] - b0[1])
            if rep >= WARMUP:
                times[name].append(ms)
            say(f"  {'warm' if rep < WARMUP else 'rep '} {rep} {name}: {ms:.1f} ms")
    inner = layer[bs:-bs, bs:-bs, bs:-bs]
    same = all(np.array_equal(inner[x].view(np.uint64), box[x].view(np.uint64)) for x in range(N))
    check(lib.gcmx_download(ctx.ptr, layer_p))  # the layer after the last write_box
    same = same and all(np.array_equal(inner[x].view(np.uint64), box[x].view(np.uint64)) for x in range(N))
    if not same:
        print("bench_state: the box and the layer differ", file=sys.stderr)
        return None, False
    calls = {k: dict(stats(v), bytes_moved=int(moved[k])) for k, v in times.items()}
    pairs = {"read": [d / r for d, r in zip(times["download"], times["read_box"])],
             "write": [u / w for u, w in zip(times["upload"], times["write_box"])]}
    calls["ratio_download_over_read_box"] = pairs["read"]
    calls["ratio_upload_over_write_box"] = pairs["write"]
    calls["gate_every_pair_faster"] = bool(all(r > 1.0 for v in pairs.values() for r in v))
    calls["rss_peak_bytes_whole_run"] = rss_peak()

    # ---- the kernels alone
    nbytes = n * 2 * M * 8
    ctx.profile(True)
    ctx.profile_reset()
    ceiling = []
    for _ in range(REPS):
        check(lib.gcmx_read_box(ctx.ptr, lo, hi, box_p, stage))
        check(lib.gcmx_write_box(ctx.ptr, lo, hi, box_p, stage))
        ceiling.append(ctx.copy_ceiling_ms(nbytes, 1))
    ctx.sync()
    prof = ctx.profile_read()
    ceiling_ms = sorted(ceiling)[len(ceiling) // 2]
    kernels = {"algorithmic_bytes": nbytes, "copy_ceiling_ms": ceiling_ms, "copy_ceiling_all_ms": ceiling,
               "copy_ceiling_tbps": nbytes / ceiling_ms / 1e9}
    for name in ("state_pack", "state_unpack"):
        p = prof[name]
        ms = p["total_ms"] / REPS
        kernels[name] = {"ms_per_box": ms, "launches_per_box": p["launches"] // REPS, "tbps": nbytes / ms / 1e9,
                         "ratio_to_ceiling": ceiling_ms / ms}
    ctx.close()
    return {"rss": rss, "calls": calls, "kernels": kernels}, rss["gate_no_box_sized_allocation"] and calls["gate_every_pair_faster"]


def engine_run(a):
    from gcm_amd import _gcm_host as H
    N = a.n
    need = N ** 3 * M * 8 + (1 << 20)
    where = a.dir or tempfile.gettempdir()
    free = shutil.disk_usage(where).free
    if free < need * 1.1:
        return {"skipped": f"the file needs {need / 2**30:.1f} GiB, {where} has {free / 2**30:.1f} GiB free"}
    t = H.Task()
    t.dimensionality = 3
    t.border_size = 2
    t.h = [1.0, 1.0, 1.0]
    t.courant = 0.9
    t.number_of_snaps = 1
    t.add_body(0, [N, N, N], [0, 0, 0])
    t.set_default_material(4.0, 2.0, 1.0)
    t.add_initial_quantity(("sphere", N / 8, (N / 2,) * 3), "PRESSURE", 10.0)
    t.set_device_setup(True)
    he = H.Engine(t)
    he.run_steps(1)
    he.sync(0)
    rss0 = rss_peak()
    out = {}
    with tempfile.TemporaryDirectory(dir=where) as tmp:
        path = os.path.join(tmp, "state.gcmx")
        done = threading.Event()

        def progress():  # a long save says how far it is (save_state and load_state release the GIL)
            while not done.wait(30.0):
                size = max((os.path.getsize(p) for p in (path + ".tmp", path) if os.path.exists(p)), default=0)
                say(f"  engine {N}^3: {size / 2**30:.1f} GiB on disk")
        threading.Thread(target=progress, daemon=True).start()
        try:
            t0 = time.perf_counter()
            he.save_state(path)
            out["save_s"] = time.perf_counter() - t0
            out["file_bytes"] = os.path.getsize(path)
            t0 = time.perf_counter()
            he.load_state(path)
            out["load_s"] = time.perf_counter() - t0
        finally:
            done.set()
    he.run_steps(1)
    he.sync(0)
    out["steps"] = he.steps
    out["rss_peak_growth_bytes"] = rss_peak() - rss0
    out["bytes_moved"] = list(he.transfer_bytes(0))
    say(f"  engine {N}^3: save {out['save_s']:.1f} s, load {out['load_s']:.1f} s, {out['file_bytes'] / 2**30:.1f} GiB")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True, help="grid size (N^3 nodes)")
    ap.add_argument("--stage-mib", type=int, default=0, help="stage_bytes of the box calls (0: the default, 256 MiB)")
    ap.add_argument("--engine", action="store_true", help="also save_state / load_state of an engine")
    ap.add_argument("--engine-only", action="store_true", help="only that")
    ap.add_argument("--dir", default="", help="where the engine's file goes (default: the temporary directory)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    try:
        import torch
        have_gpu = torch.cuda.device_count() > 0
    except Exception:
        have_gpu = False
    if not have_gpu:
        print("bench_state: no GPU", file=sys.stderr)
        return 2
    import gcm_amd

    res = {"bench": "state", "n": a.n, "border_size": 2, "M": M, "stage_mib": a.stage_mib or 256, "warmup": WARMUP,
           "reps": REPS}
    ok = True
    if not a.engine_only:
        part, ok = calls_and_kernels(a, gcm_amd)
        if part is None:
            return 1
        res.update(part)
    if a.engine or a.engine_only:
        res["engine"] = engine_run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
