"""The exact fp64 state by boxes (gcmx_read_box / gcmx_write_box, k_state_pack /
k_state_unpack) against the whole-layer calls download() / upload(), which the
parity suites hold to the oracle.  Every comparison is on bit patterns: the
states are random 64-bit words viewed as float64, so NaNs with payloads, -0.0,
infinities and subnormals all occur, and a move that is not a pure move shows."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = 1
# (sizes, borderSize): the smallest shapes that cross every edge of a 64-node tile
GRIDS = [([5, 7, 70], 2), ([4, 6, 65], 2), ([3, 5, 130], 1), ([4, 5, 63], 3), ([21, 70], 2), ([100], 2),
         ([2, 3, 1024], 2)]
LAYOUTS = {"default": {},
           "odd": {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"},
           "padded": {"GCMX_ROW_PAD": "16", "GCMX_PLANE_PAD": "64"}}
CASES = [(s, bs, "default") for s, bs in GRIDS] + [(s, bs, l) for s, bs in GRIDS[:3] for l in ("odd", "padded")]


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint64) != want.view(np.uint64)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {at}: "
                             f"got {got[at]!r} want {want[at]!r}")


@functools.lru_cache(maxsize=None)
def random_bits(shape, seed):
    """Random 64-bit patterns as float64, with the special values planted too."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    special = np.array([0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000,
                        0xFFF0000000000000, 0x7FF0000000000001, 0xFFF8DEADBEEF0001, 0x7FFFFFFFFFFFFFFF],
                       dtype=np.uint64)
    flat[rng.choice(flat.size, size=min(flat.size, 4 * special.size), replace=False)] = np.resize(special, min(flat.size, 4 * special.size))
    out = a.view(np.float64)
    out.setflags(write=False)
    return out


def boxes_for(sizes, bs, reach):
    """(name, lo, hi) per box; `reach`: how far a box may go into the ghosts (bs
    for reads, 0 for writes)."""
    D, F = len(sizes), len(sizes) - 1
    full_lo, full_hi = [0] * D, list(sizes)
    out = [("inner", full_lo, full_hi)]
    if reach:
        out.append(("all nodes", [-bs] * D, [s + bs for s in sizes]))
    mid = [s // 2 for s in sizes]
    out.append(("one node", mid, [m + 1 for m in mid]))

    def along_f(lo_f, hi_f):
        lo, hi = list(full_lo), list(full_hi)
        lo[F], hi[F] = lo_f, hi_f
        return lo, hi
    out.append(("unaligned tile",) + along_f(3, min(3 + 64, sizes[F] + reach)))
    if sizes[F] >= 65:
        out.append(("one node into a second tile",) + along_f(0, 65))
    elif reach and sizes[F] + 2 * reach >= 65:
        out.append(("one node into a second tile",) + along_f(-reach, 65 - reach))
    for d in range(D):
        lo, hi = list(full_lo), list(full_hi)
        lo[d], hi[d] = mid[d], mid[d] + 1
        out.append((f"one node thick along {d}", lo, hi))
    return out


def stage_values(ctx, lo, hi):
    """0 (the default), one row of the box plus 8 bytes (a chunk per row), two
    rows plus 8 bytes (the odd row counts are no multiple of the chunk)."""
    row = (hi[-1] - lo[-1]) * ctx.M * 8
    return [0, row + 8, 2 * row + 8]


def index_of(lo, hi, bs):
    return tuple(slice(a + bs, b + bs) for a, b in zip(lo, hi))


def make_ctx(G, monkeypatch, sizes, bs, model, layout):
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    return G.Context(len(sizes), bs, sizes, model=model)


@pytest.mark.parametrize("model", ["elastic", "acoustic"])
@pytest.mark.parametrize("sizes,bs,layout", CASES)
def test_read_box_equals_download(G, monkeypatch, sizes, bs, layout, model):
    ctx = make_ctx(G, monkeypatch, sizes, bs, model, layout)
    state = random_bits(ctx.shape_all + (ctx.M,), 1)
    ctx.upload(state)
    layer = ctx.download().reshape(state.shape)
    same_bits(layer, state, "download() of the uploaded words")
    for name, lo, hi in boxes_for(sizes, bs, bs):
        want = layer[index_of(lo, hi, bs)]
        assert want.size > 0
        for stage in stage_values(ctx, lo, hi):
            before = ctx.transfer_bytes()
            got = ctx.read_box(lo, hi, stage_bytes=stage)
            after = ctx.transfer_bytes()
            same_bits(got, want, f"{name} {lo}..{hi} stage {stage} {sizes} {model} {layout}")
            assert after[0] - before[0] == want.size * 8 and after[1] == before[1], (name, stage)
    # into a caller's array, and the all-nodes box is download() itself
    out = np.empty(state.shape)
    ctx.read_box([-bs] * len(sizes), [s + bs for s in sizes], out=out)
    same_bits(out.reshape(-1, ctx.M), ctx.download(), "all-nodes box vs download()")
    ctx.close()


@pytest.mark.parametrize("model", ["elastic", "acoustic"])
@pytest.mark.parametrize("sizes,bs,layout", CASES)
def test_write_box_replaces_the_box_only(G, monkeypatch, sizes, bs, layout, model):
    ctx = make_ctx(G, monkeypatch, sizes, bs, model, layout)
    state = random_bits(ctx.shape_all + (ctx.M,), 1)
    values = random_bits(ctx.shape_all + (ctx.M,), 2)
    for name, lo, hi in boxes_for(sizes, bs, 0):
        idx = index_of(lo, hi, bs)
        for stage in stage_values(ctx, lo, hi):
            ctx.upload(state)
            before = ctx.transfer_bytes()
            ctx.write_box(lo, values[idx], stage_bytes=stage)
            after = ctx.transfer_bytes()
            want = state.copy()
            want[idx] = values[idx]
            same_bits(ctx.download().reshape(state.shape), want,
                      f"{name} {lo}..{hi} stage {stage} {sizes} {model} {layout}")
            assert after[1] - before[1] == values[idx].size * 8 and after[0] == before[0], (name, stage)
    ctx.close()


def iso_tables(D, materials):
    t = [O.isotropic_elastic_matrices(D, *m) for m in materials]
    return np.stack([x[0] for x in t]), np.stack([x[1] for x in t]), np.stack([x[2] for x in t])


def test_write_box_keeps_the_path_and_steps_like_upload(G):
    """A context that takes the one-pass step still does after write_box, and its
    step is the step of a context that got the same state by upload()."""
    sizes, bs = [6, 9, 70], 2
    rng = np.random.default_rng(7)
    res = {}
    for mode in (G.FP_EXACT, G.FP_FMA):
        ctxs = [G.Context(3, bs, sizes) for _ in range(2)]
        state = np.zeros(ctxs[0].shape_all + (9,))
        state[2:-2, 2:-2, 2:-2] = rng.uniform(-1, 1, size=tuple(sizes) + (9,))
        new = rng.uniform(-1, 1, size=(4, 5, 66, 9))
        want = state.copy()
        want[2 + 1:2 + 5, 2 + 3:2 + 8, 2 + 2:2 + 68] = new
        for c in ctxs:
            c.set_materials(*iso_tables(3, [(4.0, 2.0, 1.0)]))
            c.fp_mode = mode
        a, b = ctxs
        a.upload(state)
        path = a.effective_path
        assert path == "fused"
        a.write_box([1, 3, 2], new, stage_bytes=66 * 9 * 8 * 3 + 8)
        assert a.effective_path == path
        b.upload(want)
        same_bits(a.download(), b.download(), "before the step")
        a.step(0.2)
        b.step(0.2)
        assert a.effective_path == b.effective_path == path
        same_bits(a.download(), b.download(), f"after the step, fp mode {mode}")
        res[mode] = a.download()
        a.close()
        b.close()
    assert np.isfinite(res[G.FP_EXACT]).all() and np.any(res[G.FP_EXACT] != 0)


def test_refusals_change_nothing(G):
    sizes, bs = [5, 7, 70], 2
    ctx = G.Context(3, bs, sizes)
    state = random_bits(ctx.shape_all + (9,), 3)
    ctx.upload(state)
    L, ptr = G.lib(), ctx._ptr
    i3 = lambda v: (ctypes.c_int * 3)(*v)
    dp = ctypes.POINTER(ctypes.c_double)
    buf = np.zeros(state.size)
    p = buf.ctypes.data_as(dp)
    before = ctx.transfer_bytes()
    refused = [
        ("empty read box", L.gcmx_read_box, [0, 0, 4], [5, 7, 4], p),
        ("inverted read box", L.gcmx_read_box, [3, 0, 0], [2, 7, 70], p),
        ("read box past sizes + bs", L.gcmx_read_box, [0, 0, 0], [5, 7, 70 + bs + 1], p),
        ("read box below -bs", L.gcmx_read_box, [-bs - 1, 0, 0], [5, 7, 70], p),
        ("null read buffer", L.gcmx_read_box, [0, 0, 0], [5, 7, 70], None),
        ("empty write box", L.gcmx_write_box, [0, 2, 0], [5, 2, 70], p),
        ("write box at -1", L.gcmx_write_box, [0, -1, 0], [5, 7, 70], p),
        ("write box into the upper ghosts", L.gcmx_write_box, [0, 0, 0], [5, 7, 71], p),
        ("null write buffer", L.gcmx_write_box, [0, 0, 0], [5, 7, 70], None),
    ]
    for what, call, lo, hi, arg in refused:
        assert call(ptr, i3(lo), i3(hi), arg, 0) == ERR_INVALID_ARG, what
    with pytest.raises(G.gcmx.GcmxError) as err:
        ctx.write_box([0, 0, 6], np.zeros((5, 7, 65, 9)))
    assert err.value.status == ERR_INVALID_ARG
    assert ctx.transfer_bytes() == before
    assert not buf.any()
    same_bits(ctx.download().reshape(state.shape), state, "the layer after the refusals")
    ctx.close()
