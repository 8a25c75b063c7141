"""Padding is neither used nor written on acoustic contexts: the method of
tests/test_gpu_poison.py (through tests/rawlayer.py) on k_step_acoustic and on
the 2-D generic stages.  Every launch runs three steps twice from the same
state, clean and with a large finite sentinel (1.5e300) in every non-node
element of both layers, with the default strides and with strides the sizes do
not imply (odd pads 3 / 5 / 7, even pads 16 / 64):

  1. the poisoned run's nodes equal the clean run's bit for bit after every step;
  2. every non-node element of both layers still holds the sentinel after the last;
  3. the clean run equals the oracle (IEEE equality), so the pair is anchored."""
import numpy as np
import pytest

from tests import acoustic_ref as A
from tests import rawlayer, states

pytestmark = pytest.mark.gpu

STEPS = 3
RHO, LAM, C = 2.0, 8.0, 2.0
H_A = (0.5, 0.4, 0.3)
PADS = {"none": {},
        "odd": {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"},
        "even": {"GCMX_ROW_PAD": "16", "GCMX_PLANE_PAD": "64"}}
# name: (sizes, bs, h, tau or None for Courant 0.9, the kernel the profile must name)
LAUNCHES = {
    "bs2-4x5x64": ([4, 5, 64], 2, H_A, None, "k_step_acoustic<2, 64, KF0>"),
    "bs2-6x9x37": ([6, 9, 37], 2, H_A, None, "k_step_acoustic<2, 64, KF0>"),
    "bs3-5x7x20": ([5, 7, 20], 3, H_A, None, "k_step_acoustic<3, 64, KF0>"),
    "!kf0-bs2-6x9x37": ([6, 9, 37], 2, (1.0, 1.0, 1.0), 1.0 / C, "k_step_acoustic<2, 64, !KF0>"),
    "2d-generic-bs2-15x11": ([15, 11], 2, H_A, None, "k_stage_generic"),
}


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


def first_difference(got, want):
    diff = got.view(np.uint64) != want.view(np.uint64)
    i0 = tuple(int(v) for v in np.argwhere(diff)[0])
    return f"{int(diff.sum())} values differ; first at {i0}: got {got[i0]!r} want {want[i0]!r}"


@pytest.mark.parametrize("pads", list(PADS))
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_padding_is_neither_read_nor_written(G, monkeypatch, name, pads):
    for k, v in PADS[pads].items():
        monkeypatch.setenv(k, v)
    sizes, bs, h, tau, kernel = LAUNCHES[name]
    D = len(sizes)
    body = A.acoustic_body(D, bs, sizes, h=h[:D], rho=RHO, lam=LAM)
    states.uniform(body, seed=sum(map(ord, name)))
    tau = 0.9 * min(body.h[:D]) / body.maximal_eigenvalue if tau is None else tau
    clean, dirty = A.context_for(body), A.context_for(body)
    g = dirty.geometry()
    if pads == "odd":
        assert g["stride"][D - 2] % 2 == 1 and g["cs"] % 2 == 1, g
    for c in (clean, dirty):
        c.profile(True)
    rawlayer.current_layer(dirty)  # the node mask reproduces gcmx_download
    mask = rawlayer.poison(dirty)
    assert not rawlayer.padding_changed(dirty, mask)
    rawlayer.current_layer(dirty)  # and poisoning changed no node
    for step in range(STEPS):
        A.step(body, tau)
        clean.step(tau)
        dirty.step(tau)
        x, y = clean.download(), dirty.download()
        what = f"{name} pads {pads} step {step}"
        assert np.isfinite(y).all(), f"{what}: the poisoned run has non-finite values"
        assert np.array_equal(y.view(np.uint64), x.view(np.uint64)), \
            f"{what}: the result depends on padding: {first_difference(y, x)}"
        assert np.array_equal(x, body.pde), f"{what}: clean run against the oracle: {first_difference(x, body.pde)}"
    for layer, where in rawlayer.padding_changed(dirty, mask).items():
        raise AssertionError(f"{name} pads {pads}: {where.size} padding elements of layer {layer} were written; "
                             f"first: {rawlayer.describe_element(dirty, where[0])}")
    rawlayer.current_layer(dirty)
    for c in (clean, dirty):
        names = [v["kernel"] for v in c.profile_read().values() if v["launches"] > 0 and v["kernel"]]
        assert names == [kernel], names
        c.close()


def test_a_value_read_for_a_ghost_is_noticed(G):
    """The pair has teeth: the sentinel in ONE x ghost the step does read changes
    the result, as it would read from a pad."""
    sizes, bs, h, tau, _ = LAUNCHES["bs2-6x9x37"]
    body = A.acoustic_body(3, bs, sizes, h=h, rho=RHO, lam=LAM)
    states.uniform(body, seed=7)
    tau = 0.9 * min(h) / body.maximal_eigenvalue
    clean, dirty = A.context_for(body), A.context_for(body)
    ghost = (bs - 1,) + tuple(s // 2 + bs for s in sizes[1:])
    e = rawlayer.node_elements(dirty).reshape(tuple(dirty.shape_all) + (dirty.M,))[ghost + (0,)]
    for w in "ab":
        raw = rawlayer.read_layer(dirty, w)
        assert raw[e] == 0.0
        raw[e] = rawlayer.SENTINEL
        rawlayer.write_layer(dirty, w, raw)
    clean.step(tau)
    dirty.step(tau)
    a = clean.download().reshape(tuple(clean.shape_all) + (clean.M,))
    b = dirty.download().reshape(a.shape)
    inner = tuple(slice(bs, -bs) for _ in sizes)
    assert not np.array_equal(a[inner], b[inner])
    clean.close()
    dirty.close()
