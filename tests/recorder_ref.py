"""The point recorder's rule (include/gcmx.h, gcmx_recorder_create_points) restated
in numpy: corners, weights and the blend in the library's operation order, in
float64, every product and every sum rounded on its own.  Nothing here comes
from the code under test."""
import numpy as np

PRESSURE = 12


def sigma(D, i, j):
    """Component of s_ij (i <= j) in the elastic PDE vector."""
    return D + i * D - ((i - 1) * i) // 2 + j - i


def quantity(model, D, code, v):
    """getQuantityOf on rows v [n, M] with the host's roundings (the elastic PRESSURE:
    trace = 0.0; trace += s_dd in order; -trace / D)."""
    if code >= 64:
        return v[:, code - 64]
    if code in (2, 3, 4):
        return v[:, code - 2]
    if model == "acoustic":
        assert code == PRESSURE
        return v[:, D]
    if code == PRESSURE:
        trace = np.zeros(len(v))
        for d in range(D):
            trace = trace + v[:, sigma(D, d, d)]
        return -trace / float(D)
    ij = {5: (0, 0), 6: (0, 1), 7: (0, 2), 8: (1, 1), 9: (1, 2), 10: (2, 2)}[code]
    return v[:, sigma(D, *ij)]


def corners(sizes, pos):
    """Base index [dim] and the 2^dim weights of one position (inner-index units).
    None: the position is refused."""
    dim = len(sizes)
    base, t = [], []
    for d in range(dim):
        p = float(pos[d])
        if sizes[d] < 2 or not (0.0 <= p <= float(sizes[d] - 1)):
            return None
        i = min(int(np.floor(p)), sizes[d] - 2)
        base.append(i)
        t.append(np.float64(p) - np.float64(i))
    w = []
    for k in range(1 << dim):
        acc = None
        for d in range(dim):
            bit = (k >> (dim - 1 - d)) & 1
            f = t[d] if bit else np.float64(1.0) - t[d]
            acc = f if acc is None else acc * f
        w.append(np.float64(acc))
    return base, w


def corner_index(dim, base, k):
    return tuple(base[d] + ((k >> (dim - 1 - d)) & 1) for d in range(dim))


def sample(layer, bs, model, positions, codes):
    """[n_q, n]: the recorded values of `positions` [n, dim] on `layer`
    [all-nodes shape..., M] (ghosts of width bs included)."""
    dim = layer.ndim - 1
    sizes = [s - 2 * bs for s in layer.shape[:dim]]
    out = np.empty((len(codes), len(positions)))
    for i, pos in enumerate(positions):
        base, w = corners(sizes, pos)
        rows = np.stack([layer[tuple(bs + j for j in corner_index(dim, base, k))] for k in range(1 << dim)])
        for q, code in enumerate(codes):
            v = quantity(model, dim, code, rows)
            acc = w[0] * v[0]
            for k in range(1, 1 << dim):
                acc = acc + w[k] * v[k]
            out[q, i] = acc
    return out
