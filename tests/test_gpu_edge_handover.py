"""The Z-edge hand-over between the waves of a barrier-free one-pass block
(k_step_tx2's UNI instances, `publish` / `collect`): every wave writes the 2 bs
edge columns of its Y results into a two-row ring and bumps its row counter;
its neighbours wait for the counter and copy those edges into their own halo
slots, one value per hardware lane -- lanes [0, NE) of the lower half-wave the
left neighbour's 2 (nodes) x 6 (components) x bs values, lanes [32, 32 + NE) the
right neighbour's.  The cases are the smallest shapes at which that lane-to-value
map, or its masks, can go wrong:

  Z = 128    two waves, one neighbour each (both masks), bs 1 and 2, odd and even
             X; 40 rows, so both ring rows are reused many times
  Z = 512    eight waves, z blocks dealt to SIMD partners (the wave index of the
             exchange is not the hardware wave)
  Z = 256    the two-blocks-per-CU instance (8-byte path)
  Z = 1024   the z split: parts of eight waves, cut lanes
  n8         a UNI launch on the 8-byte path (odd row / plane padding)
  het        per-node materials, bs 1 (16-byte path) and bs 2 (8-byte path)
  free6      free surfaces on all six faces: the face ghosts in wave 0's left and
             the last wave's right halo must survive the copy lanes
  plain      no faces and a state that is non-zero right up to z = 0 and
             z = Z - 1: those two halos must stay zero
  chunks     several y chunks per launch (16 rows requested), even and odd row
             counts: a downward-marching chunk, both parities of the row count

Exact build: 3 steps at Courant 0.9, bitwise equal to the oracle on the inner
nodes after every step.  FMA build: within 1e-10 relative L2 of the exact build
(the suite's FMA tolerance).  The kernel name in the profile says which instance
ran, so no case passes on another path."""
import functools

import numpy as np
import pytest

from tests.helpers import context_for, oracle_body, random_materials, random_state
from tests.test_gpu_faces import face_body, faces_at, free

pytestmark = pytest.mark.gpu

STEPS = 3
MATS = ((4.0, 2.0, 1.0), (1.0, 2.0, 0.8), (2.5, 0.0, 3.0))
TAU_HET = 0.9 / np.sqrt((3.0 + 6.0) / 2.5)  # Courant 0.9 on the fastest material
FREE_ALL = [(0, 0, free(0)), (1, 0, free(1)), (2, 0, free(2))]

# name: (kind, bs, sizes, path, instance, options); path: "wide" or "n8" (a UNI
# launch on the 8-byte path); instance: what the kernel's name must start with;
# options: rows (rows per block requested), env (set while the context is made)
CASES = {}
for _bs in (1, 2):
    CASES[f"plain-bs{_bs}-3x40x128"] = ("plain", _bs, [3, 40, 128], "wide", f"k_step_tx2<{_bs}, 128, KF0, UNI, !FACES", {})
    CASES[f"plain-bs{_bs}-4x40x128"] = ("plain", _bs, [4, 40, 128], "wide", f"k_step_tx2<{_bs}, 128, KF0, UNI, !FACES", {})
    CASES[f"plain-bs{_bs}-4x21x512"] = ("plain", _bs, [4, 21, 512], "wide", f"k_step_tx2<{_bs}, 512, KF0, UNI, !FACES", {})
    CASES[f"free6-bs{_bs}-3x40x128"] = ("faces", _bs, [3, 40, 128], "wide", f"k_step_tx2<{_bs}, 128, KF0, UNI, FACES", {})
    CASES[f"free6-bs{_bs}-4x21x512"] = ("faces", _bs, [4, 21, 512], "wide", f"k_step_tx2<{_bs}, 512, KF0, UNI, FACES", {})
    CASES[f"n8-bs{_bs}-3x40x128"] = ("plain", _bs, [3, 40, 128], "n8", f"k_step_tx2<{_bs}, 128, KF0, UNI, !FACES",
                                     {"env": {"GCMX_ROW_PAD": "1", "GCMX_PLANE_PAD": "1"}})
CASES["plain-bs2-3x12x256"] = ("plain", 2, [3, 12, 256], "n8", "k_step_tx2<2, 256, KF0, UNI, !FACES", {})
CASES["zsplit-bs2-4x12x1024"] = ("plain", 2, [4, 12, 1024], "wide", "k_step_tx2<2, 512, KF0, UNI, !FACES, ZS", {})
CASES["zsplit-bs1-4x12x1024"] = ("plain", 1, [4, 12, 1024], "wide", "k_step_tx2<1, 512, KF0, UNI, !FACES, ZS", {})
# per-node materials: the 16-byte path at borderSize 1, the 8-byte one at 2 (registers)
CASES["het-bs1-4x40x128"] = ("het", 1, [4, 40, 128], "wide", "k_step_tx2<1, 128, KF0, UNI, !FACES, HET", {})
CASES["het-bs2-3x40x128"] = ("het", 2, [3, 40, 128], "n8", "k_step_tx2<2, 128, KF0, UNI, !FACES, HET", {})
# several y chunks per launch: 16 + 16 + 8 rows, and 16 + 16 + 9
CASES["chunks-bs2-3x40x128"] = ("plain", 2, [3, 40, 128], "wide", "k_step_tx2<2, 128, KF0, UNI, !FACES", {"rows": 16})
CASES["chunks-bs2-3x41x128"] = ("plain", 2, [3, 41, 128], "wide", "k_step_tx2<2, 128, KF0, UNI, !FACES", {"rows": 16})
CASES["chunks-bs1-4x41x128"] = ("plain", 1, [4, 41, 128], "wide", "k_step_tx2<1, 128, KF0, UNI, !FACES", {"rows": 16})


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


class Case:
    """One case: the oracle body in its initial state, and how both sides step."""

    def __init__(self, name):
        self.kind, bs, sizes, self.path, self.instance, self.opt = CASES[name]
        self.tau = 0.9
        seed = sum(map(ord, name))
        if self.kind == "plain":
            self.body = oracle_body(3, bs, sizes)
        elif self.kind == "faces":
            self.body = face_body(3, bs, sizes, FREE_ALL)
        else:
            self.body = oracle_body(3, bs, sizes, materials=MATS, courant=0.9)
            random_materials(self.body, seed=seed + 1)
            self.tau = TAU_HET
        random_state(self.body, seed=seed, ghosts=False)
        # every case: the state is non-zero right up to both z faces
        inner = self.body.inner_view()
        assert np.all(inner[..., 0, :] != 0.0) and np.all(inner[..., -1, :] != 0.0)

    def oracle_step(self, t):
        b = self.body
        for s in range(3):
            if self.kind == "faces":
                b.apply_border(s, t)
            b.stage(s, self.tau)

    def context(self, G, fp, monkeypatch):
        with monkeypatch.context() as m:
            for k, v in self.opt.get("env", {}).items():
                m.setenv(k, v)
            ctx = context_for(self.body)
        if "env" in self.opt:
            g = ctx.geometry()
            assert g["stride"][0] % 2 == 1 or g["stride"][1] % 2 == 1, g
        if "rows" in self.opt:
            ctx.set_schedule(G.SCHED_AUTO, self.opt["rows"])
        ctx.fp_mode = fp
        ctx.profile(True)
        return ctx

    def gpu_step(self, ctx, t):
        if self.kind == "faces":
            ctx.step_faces(self.tau, faces_at(3, FREE_ALL, t))
        else:
            ctx.step(self.tau)
        assert ctx.last_path == "fused"

    def inner(self, ctx):
        return self.body.inner_view(ctx.download().reshape(self.body.pde.shape)).copy()

    def check_kernel(self, ctx):
        k = ctx.profile_read()["fused_xyz"]["kernel"]
        assert k.startswith(self.instance), f"{self.instance}...> expected, ran {k}"
        assert "!UNI" not in k, k
        ran = "n8" if ", N8" in k else "wide"
        assert ran == self.path, f"{self.path} path expected, ran {k}"
        return k


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
def test_exact_build_equals_oracle(G, monkeypatch, name):
    c = Case(name)
    want = oracle_steps(name)
    ctx = c.context(G, G.FP_EXACT, monkeypatch)
    t = 0.0
    for step in range(STEPS):
        c.gpu_step(ctx, t)
        assert_bitwise(c.inner(ctx), want[step], f"{name} step {step}")
        t += c.tau
    c.check_kernel(ctx)
    ctx.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fma_build_within_tolerance_of_exact(G, monkeypatch, name):
    c = Case(name)
    ex = c.context(G, G.FP_EXACT, monkeypatch)
    fm = c.context(G, G.FP_FMA, monkeypatch)
    t = 0.0
    for step in range(STEPS):
        c.gpu_step(ex, t)
        c.gpu_step(fm, t)
        want, got = c.inner(ex), c.inner(fm)
        r = float(np.linalg.norm(got - want)) / float(np.linalg.norm(want))
        print(f"{name} step {step}: FMA against exact, relative L2 {r:.3e}")
        assert r <= 1e-10, f"{name} step {step}: relative L2 {r:.3e} > 1e-10"
        t += c.tau
    assert "FMA" in c.check_kernel(fm)
    c.check_kernel(ex)
    for x in (ex, fm):
        x.close()
