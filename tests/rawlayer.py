"""Raw device memory of a context's two time layers (tests only).

gcmx_download returns the nodes of the current layer and nothing else: the row
lead, the row / plane / component padding and the layer that is not current
never reach the host.  This module reads and writes whole layers with hipMemcpy
on the HIP runtime libgcmx.so is linked against (the copy this process has
already mapped; never a second one), and knows which elements of a layer are
nodes:

    element(c, x, y, z) = c cs + origin + (x - bs) s0 + (y - bs) s1 + (z - bs) s2

for every ghost-padded index (gcmx_geometry).  Everything else is padding."""
import ctypes

import numpy as np

SENTINEL = 1.5e300  # finite on purpose: DESIGN.md §3.5 (min / max drop a NaN)
_H2D, _D2H = 1, 2
_hip = None


def hip():
    """The HIP runtime as mapped by libgcmx.so."""
    global _hip
    if _hip is not None:
        return _hip
    import gcm_amd
    gcm_amd.lib()
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            fields = line.split(None, 5)  # address perms offset dev inode path
            if len(fields) == 6 and "libamdhip64.so" in fields[5]:
                paths.add(fields[5].strip())
    if len(paths) != 1:
        raise RuntimeError(f"expected one mapped HIP runtime, found {sorted(paths)}")
    h = ctypes.CDLL(paths.pop())
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipMemcpy.restype = ctypes.c_int
    _hip = h
    return h


def node_elements(ctx) -> np.ndarray:
    """Element offsets of every node in gcmx_download's order: [n_all, M]."""
    g = ctx.geometry()
    off = np.full((1,) * ctx.dim, g["origin"], dtype=np.int64)
    for i, n in enumerate(ctx.shape_all):
        shape = [1] * ctx.dim
        shape[i] = n
        off = off + ((np.arange(n, dtype=np.int64) - ctx.bs) * g["stride"][i]).reshape(shape)
    return off.reshape(-1, 1) + np.arange(ctx.M, dtype=np.int64) * g["cs"]


def layer_elements(ctx) -> int:
    return ctx.layer_info()["layer_bytes"] // 8


def node_mask(ctx) -> np.ndarray:
    """True at the elements of a layer that hold a node (inner or ghost)."""
    idx = node_elements(ctx)
    n = layer_elements(ctx)
    assert idx.min() >= 0 and idx.max() < n, (int(idx.min()), int(idx.max()), n)
    mask = np.zeros(n, dtype=bool)
    mask[idx.reshape(-1)] = True
    assert int(mask.sum()) == idx.size, "two nodes share an element"
    return mask


def read_layer(ctx, which: str) -> np.ndarray:
    """Layer "a" or "b" as it lies in device memory."""
    ctx.sync()
    info = ctx.layer_info()
    out = np.empty(info["layer_bytes"] // 8)
    rc = hip().hipMemcpy(out.ctypes.data, info[which], info["layer_bytes"], _D2H)
    assert rc == 0, f"hipMemcpy device to host: error {rc}"
    return out


def write_layer(ctx, which: str, raw: np.ndarray):
    ctx.sync()
    info = ctx.layer_info()
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    assert raw.nbytes == info["layer_bytes"]
    rc = hip().hipMemcpy(info[which], raw.ctypes.data, info["layer_bytes"], _H2D)
    assert rc == 0, f"hipMemcpy host to device: error {rc}"


def current_layer(ctx) -> str:
    """Self-check of the node mask: the elements under it, reordered, are
    gcmx_download's array, bit for bit, in exactly one way.  Returns which layer
    holds the state ("a" or "b"; "ab" when both hold the same bits)."""
    idx = node_elements(ctx)
    want = ctx.download().view(np.uint64)
    hit = "".join(w for w in "ab" if np.array_equal(read_layer(ctx, w)[idx].view(np.uint64), want))
    assert hit, "neither raw layer holds gcmx_download's nodes under the node mask"
    return hit


def poison(ctx, value: float = SENTINEL) -> np.ndarray:
    """Write `value` into every non-node element of both layers; returns the mask."""
    mask = node_mask(ctx)
    for w in "ab":
        raw = read_layer(ctx, w)
        raw[~mask] = value
        write_layer(ctx, w, raw)
    return mask


def padding_changed(ctx, mask: np.ndarray, value: float = SENTINEL) -> dict:
    """Per layer, the offsets of non-node elements whose bits are not `value`'s."""
    bits = np.array([value]).view(np.uint64)[0]
    out = {}
    for w in "ab":
        raw = read_layer(ctx, w).view(np.uint64)
        bad = np.flatnonzero(~mask & (raw != bits))
        if bad.size:
            out[w] = bad
    return out


def describe_element(ctx, e: int) -> str:
    """Where a padding element lies: component, x plane, row, column."""
    g = ctx.geometry()
    c, r = divmod(int(e), g["cs"])
    s = g["stride"]
    if ctx.dim == 3:
        x, r2 = divmod(r, s[0])
        y, z = divmod(r2, s[1])
        return f"component {c}, plane {x}, row {y}, column {z} of {g['row']} (plane stride {s[0]}, row stride {s[1]})"
    if ctx.dim == 2:
        x, y = divmod(r, s[0])
        return f"component {c}, row {x}, column {y} of {g['row']}"
    return f"component {c}, element {r}"
