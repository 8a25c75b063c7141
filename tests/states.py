"""Deterministic states the random parity data never produces: a lone impulse
in a quiescent medium, piecewise-constant blocks (equal neighbours, exactly zero
differences, a jump at every cut; for rows longer than 512 also with the last
cut on the part cut), a linear ramp (second differences exactly
zero) and the random state scaled by a power of two far from 1 (subnormals
included).  Every family fills the inner nodes only: ghosts stay zero, so the
one-pass paths stay eligible."""
import numpy as np

STEP_VALUES = (1.0, -0.5, 0.25, 0.0)
SCALES = (-1000, 1000, -1060)


def _inner(body):
    body.pde[:] = 0.0
    return body.inner_view()


Z_PART = 512  # rows longer than this run as parts of Z_PART lanes, cut at every multiple


def z_cut(body):
    """Where the last axis is cut: the wave seam (64) of rows of 128 and more."""
    n = body.sizes[body.D - 1]
    return 64 if (body.D == 3 and n >= 128) else n // 2


def impulse_nodes(body):
    """name -> inner index of the placements this body has."""
    n = body.sizes[:body.D]
    centre = tuple(s // 2 for s in n)
    out = {"centre": centre, "first": (0,) * body.D, "last": tuple(s - 1 for s in n)}
    if body.D == 3 and n[2] >= 128:
        out["z63"] = centre[:2] + (63,)
        out["z64"] = centre[:2] + (64,)
    if body.D == 3 and n[2] > Z_PART:
        # both sides of the part cut, and the columns that at borderSize 2 lie just
        # outside the 2 bs columns the seam kernel stores (510 .. 513): the parts
        # store them, the seam kernel's group of 4 bs columns reads them
        for z in (Z_PART - 1, Z_PART, Z_PART - 3, Z_PART + 2):
            out[f"z{z}"] = centre[:2] + (z,)
    return out


def impulse(body, where="centre"):
    """Zero except one node, whose components are 1 .. M."""
    v = _inner(body)
    node = impulse_nodes(body)[where]
    v[node] = np.arange(1, body.M + 1, dtype=np.float64)
    return node


def steps(body, last_cut=None):
    """Piecewise constant over the 2^D blocks cut at X // 2, Y // 2 and z_cut (or
    `last_cut`); the value of block o and component c is
    STEP_VALUES[(o + (o >> 2) + c) % 4], which differs across every cut."""
    v = _inner(body)
    D = body.D
    cuts = [body.sizes[i] // 2 for i in range(D - 1)] + [z_cut(body) if last_cut is None else last_cut]
    o = np.zeros(v.shape[:D], dtype=np.int64)
    for i in range(D):
        shape = [1] * D
        shape[i] = body.sizes[i]
        o = o + ((np.arange(body.sizes[i]) >= cuts[i]).astype(np.int64) << (D - 1 - i)).reshape(shape)
    vals = np.array(STEP_VALUES)
    for c in range(body.M):
        v[..., c] = vals[(o + (o >> 2) + c) % 4]


def steps_zcut(body):
    """`steps` with the last cut on the part cut of rows longer than Z_PART: the
    jump and the limiter ties lie on the columns the seam kernel recomputes."""
    assert body.D == 3 and body.sizes[2] > Z_PART
    steps(body, last_cut=Z_PART)


def ramp(body):
    """(i + 2 j + 3 k + c) / 8: exact in double, second differences exactly zero."""
    v = _inner(body)
    D = body.D
    s = np.zeros(v.shape[:D])
    for i in range(D):
        shape = [1] * D
        shape[i] = body.sizes[i]
        s = s + ((i + 1.0) * np.arange(body.sizes[i])).reshape(shape)
    for c in range(body.M):
        v[..., c] = (s + c) * 0.125


def uniform(body, seed=0x57A7E):
    v = _inner(body)
    v[...] = np.random.default_rng(seed).uniform(-1, 1, v.shape)


def scaled(body, e, seed=0x57A7E):
    """The uniform(-1, 1) state times 2^e."""
    uniform(body, seed)
    body.pde[:] = np.ldexp(body.pde, e)


def taint(body, node, variant):
    """The uniform state with one inner node tainted: "vx-nan", "s-nan" (the last
    stress component) or "vx-inf"."""
    uniform(body)
    comp, val = {"vx-nan": (0, np.nan), "s-nan": (body.M - 1, np.nan), "vx-inf": (0, np.inf)}[variant]
    body.inner_view()[tuple(node) + (comp,)] = val


def canonical_bits(a):
    """IEEE equality with +0 and -0 identified, as bits."""
    return (np.asarray(a) + 0.0).view(np.uint64)


def sign_differing_zeros(got, want):
    z = (got == 0.0) & (want == 0.0)
    return int(np.sum(z & (np.signbit(got) != np.signbit(want))))
