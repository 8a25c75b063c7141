"""The one-pass step's 16-byte path (k_step_tx2's UNI instances): in the barrier-free
instances (Z == ZT, a multiple of 64) lane l < 32 of a wave owns column 2l of
its 64-column block and lane l + 32 column 2l + 1; loads and stores move column
pairs and a half-wave swap sorts them into the lanes.  Every place that maps a
lane to a column is covered here: one wave with both row ends (Z = 64), the edge
ring between waves (128), the dealing of blocks to SIMD partners (512), the z
split (1024), odd plane counts, Y = 2 bs + 1, a range starting on a node that is
not ours, both border sizes, face ghosts (uniform and per-node maps) and
per-node materials.  Launches that cannot take the path (Z < ZT; rows or planes
at odd elements) must keep the 8-byte one.  The kernel name in the profile says
which ran: a UNI instance runs the 16-byte path unless its name carries ", N8";
the !UNI instances (Z < ZT) have the 8-byte path only.

Exact build: 3 steps at Courant 0.9, bitwise equal to the oracle on the inner
nodes after every step.  FMA build: the same cases within 1e-10 relative L2 of
the exact build (both run side by side; the FMA tolerance of the suite)."""
import functools

import numpy as np
import pytest

from tests.helpers import context_for, oracle_body, random_materials, random_state
from tests.test_gpu_faces import (PARTIAL_CASES, conditions_at, face_body, face_maps, faces_at, free,
                                  partial_body)

pytestmark = pytest.mark.gpu

STEPS = 3
MATS = ((4.0, 2.0, 1.0), (1.0, 2.0, 0.8), (2.5, 0.0, 3.0))
TAU_HET = 0.9 / np.sqrt((3.0 + 6.0) / 2.5)  # Courant 0.9 on the fastest material
FREE_ALL = [(0, 0, free(0)), (1, 0, free(1)), (2, 0, free(2))]

# name: (kind, bs, sizes, start, path): "wide", "n8" (a UNI launch on the 8-byte
# path) or "!uni" (idle lanes: the 8-byte instances)
CASES = {}
for _bs in (1, 2):
    for _z in (64, 128, 512):
        CASES[f"plain-bs{_bs}-3x6x{_z}"] = ("plain", _bs, [3, 6, _z], [0, 0, 0], "wide")
        CASES[f"plain-bs{_bs}-4x5x{_z}"] = ("plain", _bs, [4, 5, _z], [0, 0, 0], "wide")
    CASES[f"start1-bs{_bs}-4x5x64"] = ("plain", _bs, [4, 5, 64], [1, 0, 0], "wide")
    CASES[f"start1-bs{_bs}-3x6x128"] = ("plain", _bs, [3, 6, 128], [1, 0, 0], "wide")
    CASES[f"free6-bs{_bs}-4x8x64"] = ("faces", _bs, [4, 8, 64], [0, 0, 0], "wide")
    CASES[f"free6-bs{_bs}-5x8x128"] = ("faces", _bs, [5, 8, 128], [0, 0, 0], "wide")
    # per-node materials: wide at borderSize 1, the 8-byte path at 2 (registers)
    CASES[f"het-bs{_bs}-5x7x64"] = ("het", _bs, [5, 7, 64], [0, 0, 0], "wide" if _bs == 1 else "n8")
    CASES[f"het-bs{_bs}-4x6x128"] = ("het", _bs, [4, 6, 128], [0, 0, 0], "wide" if _bs == 1 else "n8")
    CASES[f"zsplit-bs{_bs}-4x12x1024"] = ("plain", _bs, [4, 12, 1024], [0, 0, 0], "wide")
    CASES[f"narrow-bs{_bs}-4x6x40"] = ("plain", _bs, [4, 6, 40], [0, 0, 0], "!uni")
# 256-lane blocks (two per CU) keep the 8-byte path: the wide one measured slower there
CASES["plain-bs2-3x6x256"] = ("plain", 2, [3, 6, 256], [0, 0, 0], "n8")
CASES["facemap-mixed-10x24x64"] = ("facemap", "mixed", None, None, "wide")
CASES["facemap-bs1-7x12x64"] = ("facemap", "bs1", None, None, "wide")


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


class Case:
    """One case: the oracle body in its initial state, and how both sides step."""

    def __init__(self, name):
        kind, bs, sizes, start, self.path = CASES[name]
        self.kind, self.tau, self.conds = kind, 0.9, None
        seed = sum(map(ord, name))
        if kind == "plain":
            self.body = oracle_body(3, bs, sizes, start=start)
        elif kind == "faces":
            self.conds = FREE_ALL
            self.body = face_body(3, bs, sizes, FREE_ALL)
        elif kind == "het":
            self.body = oracle_body(3, bs, sizes, materials=MATS, courant=0.9)
            random_materials(self.body, seed=seed + 1)
            self.tau = TAU_HET
        else:
            pbs, psizes, self.conds, self.tau, path = PARTIAL_CASES[bs]
            assert path == "fused"
            self.sizes = psizes
            self.body = partial_body(pbs, psizes, self.conds)
        random_state(self.body, seed=seed, ghosts=False)

    def oracle_step(self, t):
        b = self.body
        for s in range(3):
            if self.kind in ("faces", "facemap"):
                b.apply_border(s, t)
            b.stage(s, self.tau)

    def context(self, G, fp):
        ctx = context_for(self.body)
        ctx.fp_mode = fp
        ctx.profile(True)
        self.fmap = ctx.face_map(face_maps(self.body, self.sizes)) if self.kind == "facemap" else None
        return ctx

    def gpu_step(self, ctx, t):
        if self.kind == "faces":
            ctx.step_faces(self.tau, faces_at(3, self.conds, t))
        elif self.kind == "facemap":
            ctx.step_face_map(self.tau, self.fmap, conditions_at(self.body, t))
        else:
            ctx.step(self.tau)
        assert ctx.last_path == "fused"

    def inner(self, ctx):
        return self.body.inner_view(ctx.download().reshape(self.body.pde.shape)).copy()


def kernel_of(ctx):
    return ctx.profile_read()["fused_xyz"]["kernel"]


def check_path(k, path):
    assert k.startswith("k_step_tx2<"), k
    ran = "!uni" if "!UNI" in k else "n8" if ", N8" in k else "wide"
    assert ran == path, f"{path} path expected, ran {k}"


@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    """Inner nodes of the oracle after each step (computed once per case)."""
    c = Case(name)
    out, t = [], 0.0
    for _ in range(STEPS):
        c.oracle_step(t)
        out.append(c.body.inner_view(c.body.pde).copy())
        t += c.tau
    return out


def assert_bitwise(got, want, what):
    if not np.array_equal(got, want):
        diff = got != want
        i0 = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} inner values differ; first at {i0}: "
                             f"got {got[i0]!r} want {want[i0]!r}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_build_equals_oracle(G, name):
    c = Case(name)
    want = oracle_steps(name)
    ctx = c.context(G, G.FP_EXACT)
    t = 0.0
    for step in range(STEPS):
        c.gpu_step(ctx, t)
        assert_bitwise(c.inner(ctx), want[step], f"{name} step {step}")
        t += c.tau
    check_path(kernel_of(ctx), c.path)
    ctx.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fma_build_within_tolerance_of_exact(G, name):
    c = Case(name)
    ex, fm = c.context(G, G.FP_EXACT), None
    fmap_ex = c.fmap
    fm = c.context(G, G.FP_FMA)
    fmap_fm = c.fmap
    t = 0.0
    for step in range(STEPS):
        c.fmap = fmap_ex
        c.gpu_step(ex, t)
        c.fmap = fmap_fm
        c.gpu_step(fm, t)
        want, got = c.inner(ex), c.inner(fm)
        r = float(np.linalg.norm(got - want)) / float(np.linalg.norm(want))
        print(f"{name} step {step}: FMA against exact, relative L2 {r:.3e}")
        assert r <= 1e-10, f"{name} step {step}: relative L2 {r:.3e} > 1e-10"
        t += c.tau
    k = kernel_of(fm)
    check_path(k, c.path)
    assert "FMA" in k, k
    for x in (ex, fm):
        x.close()


@pytest.mark.parametrize("pads", [{"GCMX_ROW_PAD": "1"}, {"GCMX_PLANE_PAD": "3"},
                                  {"GCMX_ROW_PAD": "1", "GCMX_PLANE_PAD": "1"}])
def test_odd_strides_take_the_narrow_path(G, monkeypatch, pads):
    """Rows or planes that start at odd elements (odd GCMX_ROW_PAD /
    GCMX_PLANE_PAD) are not 16-byte aligned: the launch keeps the 8-byte
    instance, and still equals the oracle bitwise."""
    for k, v in pads.items():
        monkeypatch.setenv(k, v)
    name = "plain-bs2-4x5x64"
    c = Case(name)
    want = oracle_steps(name)
    ctx = c.context(G, G.FP_EXACT)
    g = ctx.geometry()
    assert g["stride"][0] % 2 == 1 or g["stride"][1] % 2 == 1, g
    t = 0.0
    for step in range(STEPS):
        c.gpu_step(ctx, t)
        assert_bitwise(c.inner(ctx), want[step], f"{name} {pads} step {step}")
        t += c.tau
    check_path(kernel_of(ctx), "n8")
    ctx.close()
