"""Padding is neither used nor written.

gcmx_create zeroes both layers, so the row lead, the row / plane / component
padding and every y/z ghost of a one-pass launch all hold 0.0: a load that is
off by one element and takes the row lead for a ghost returns the right value,
and a 16-byte store that spills into a pad is never downloaded.  Here every
catalogue launch (tests/launch_catalog.py) runs twice from the same state, once
as it is and once with a large finite sentinel in every non-node element of
both layers (tests/rawlayer.py), in both floating-point builds:

  1. the poisoned run's nodes equal the clean run's bit for bit after every step;
  2. every non-node element of both layers still holds the sentinel after the last;
  3. in the exact build the clean run equals the oracle, as the parity suites
     assert it (IEEE equality), so the pair is anchored.

The sentinel is finite (1.5e300): the limiter's v_min_f64 / v_max_f64 return the
other operand for a NaN, so a NaN read by mistake can vanish
on its way to the result, while a huge finite value wins a min or a max and
swamps every sum it enters."""
import numpy as np
import pytest

from tests import rawlayer, states
from tests.launch_catalog import BY_NAME, CATALOG

pytestmark = pytest.mark.gpu

STEPS = 3
ODD_PADS = {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"}
EVEN_PADS = {"GCMX_ROW_PAD": "16", "GCMX_PLANE_PAD": "64"}
# the odd pads put k_step_tx2's UNI launches on the 8-byte path (", N8"), as
# test_odd_strides_take_the_narrow_path shows; the even ones keep the wide path
PADDED = [("tx2-wide-bs2-4x5x64", "odd"), ("tx2-!uni-bs2-4x6x40", "odd"), ("ortho-bs2-6x9x37", "odd"),
          ("2d-iso-bs2-21x70", "odd"), ("tx2-wide-bs2-4x5x64", "even"), ("acoustic-bs2-4x5x64", "odd"),
          ("tx2-faces-ode-bs2-4x8x64", "odd"), ("gp-tx2-wide-bs2-4x5x64", "odd")]


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def fp_of(G, fp):
    return {"exact": G.FP_EXACT, "fma": G.FP_FMA}[fp]


def first_difference(got, want):
    diff = got.view(np.uint64) != want.view(np.uint64)
    i0 = tuple(int(v) for v in np.argwhere(diff)[0])
    return f"{int(diff.sum())} values differ; first at {i0}: got {got[i0]!r} want {want[i0]!r}"


def run_pair(G, entry, fp):
    body = entry.body()
    states.uniform(body, seed=sum(map(ord, entry.name)))
    clean, dirty = entry.start(body, fp_of(G, fp)), entry.start(body, fp_of(G, fp))
    masks = []
    for c in dirty.ctxs:
        rawlayer.current_layer(c)  # the node mask reproduces gcmx_download
        masks.append(rawlayer.poison(c))
        assert not rawlayer.padding_changed(c, masks[-1])
        rawlayer.current_layer(c)  # and poisoning changed no node
    t = 0.0
    for step in range(STEPS):
        want = entry.oracle_step(body, t)
        a, b = clean.step(t), dirty.step(t)
        for k, (x, y, w) in enumerate(zip(a, b, want)):
            what = f"{entry.name} {fp} step {step}" + (f" stage {k}" if len(a) > 1 else "")
            assert np.isfinite(y).all(), f"{what}: the poisoned run has non-finite values"
            assert np.array_equal(y.view(np.uint64), x.view(np.uint64)), \
                f"{what}: the result depends on padding: {first_difference(y, x)}"
            if fp == "exact":
                assert np.array_equal(x, w), f"{what}: clean run against the oracle: {first_difference(x, w)}"
        t += clean.tau
    for c, mask in zip(dirty.ctxs, masks):
        bad = rawlayer.padding_changed(c, mask)
        for layer, where in bad.items():
            raise AssertionError(f"{entry.name} {fp}: {where.size} padding elements of layer {layer} were "
                                 f"written; first: {rawlayer.describe_element(c, where[0])}")
        rawlayer.current_layer(c)
    names = clean.check_kernels()
    assert dirty.check_kernels() == names
    clean.close()
    dirty.close()
    return names


@pytest.mark.parametrize("fp", ["exact", "fma"])
@pytest.mark.parametrize("entry", CATALOG, ids=repr)
def test_padding_is_neither_read_nor_written(G, entry, fp):
    names = run_pair(G, entry, fp)
    print(f"{entry.name} {fp}: {sorted(set(names))}")


@pytest.mark.parametrize("fp", ["exact", "fma"])
@pytest.mark.parametrize("name,pads", PADDED)
def test_padding_with_perturbed_strides(G, monkeypatch, name, pads, fp):
    """The same with strides the sizes do not imply: odd pads (rows and planes at
    odd elements, the 8-byte path) and, for the wide case, even ones."""
    for k, v in (ODD_PADS if pads == "odd" else EVEN_PADS).items():
        monkeypatch.setenv(k, v)
    entry = BY_NAME[name]
    if pads == "odd" and ", N8" in entry.absent:
        # rows at odd elements: the same launch on the UNI instance's 8-byte path
        entry = entry.variant(name + "-odd", entry.marks + (", N8",), tuple(m for m in entry.absent if m != ", N8"))
    dim = entry.body().D
    c = G.Context(dim, 2, [4] * dim)
    g = c.geometry()
    c.close()
    if pads == "odd":
        assert g["stride"][dim - 2] % 2 == 1 and g["cs"] % 2 == 1, g
    else:
        assert g["stride"][1] == 32 + 16 and g["stride"][0] == (32 + 16) * 8 + 64, g
    run_pair(G, entry, fp)


@pytest.mark.parametrize("name", ["tx2-wide-bs2-4x5x64", "tx2-wide-bs1-4x5x64", "tx2-!uni-bs2-4x6x40",
                                  "tx2-zs-bs2-4x12x1024", "ortho-bs2-6x9x37", "2d-iso-bs2-21x70",
                                  "acoustic-bs2-4x5x64", "tx2-faces-courant15-bs2-4x8x64", "tx2-ode-bs2-4x6x64",
                                  "gp-tx2-wide-bs2-4x5x64"])
def test_a_value_read_for_a_ghost_is_noticed(G, name):
    """The pair has teeth: the sentinel in ONE element the step does read for a
    ghost (the x ghost next to a central inner node, component 0; the y and z
    ghosts of the state a step starts from are read by no stage; the face entry
    has no condition on its x faces, whose fill would overwrite the ghost) changes
    the result, as it would read from a pad."""
    entry = BY_NAME[name]
    body = entry.body()
    states.uniform(body, seed=7)
    clean, dirty = entry.start(body, G.FP_EXACT), entry.start(body, G.FP_EXACT)
    c = dirty.ctxs[0]
    ghost = (c.bs - 1,) + tuple(s // 2 + c.bs for s in c.sizes[1:])
    e = rawlayer.node_elements(c).reshape(tuple(c.shape_all) + (c.M,))[ghost + (0,)]
    for w in "ab":
        raw = rawlayer.read_layer(c, w)
        assert raw[e] == 0.0
        raw[e] = rawlayer.SENTINEL
        rawlayer.write_layer(c, w, raw)
    a, b = clean.step(0.0)[-1], dirty.step(0.0)[-1]
    # the inner nodes of an all-nodes grid; a face or ODE entry returns them alone
    inner = tuple(slice(c.bs, -c.bs) for _ in c.sizes) if entry.compare == "all" else ()
    assert not np.array_equal(a[inner], b[inner]), f"{name}: a sentinel in the ghost {ghost} left the result unchanged"
    clean.close()
    dirty.close()


def test_largest_raw_layer_is_small(G):
    c = G.Context(3, 2, [4, 12, 1024])
    n = c.layer_info()["layer_bytes"]
    c.close()
    assert n < 10e6, n
