"""Set-up on the device: gcmx_setup_state (k_setup_state), gcmx_setup_material_ids
and gcmx_setup_census (k_setup_ids), gcmx_download_material_ids, and the engine
with Task.set_device_setup(True).

Expected values never come from the code under test: they are
_gcm_host.host_state(task, id), the CPU restatement of MaterialsCondition::apply
and InitialCondition::apply, itself held to oracle/oracle.py's set-up for the
elastic cases.  Every comparison is on the bit patterns of ALL nodes, ghosts
included."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = 1
START = (3, -2, 10)
H_STD = (0.5, 1.0, 0.25)
H_ODD = (0.1, 0.3, 0.7)
# (sizes, borderSize): odd sizes, rows of more than one 64-node segment, one row per block and many
GRIDS = [([5, 7, 70], 2), ([4, 6, 65], 2), ([3, 5, 130], 1), ([4, 5, 63], 3), ([21, 70], 2), ([100], 2)]
LAYOUTS = {"default": {},
           "odd": {"GCMX_ROW_PAD": "3", "GCMX_PLANE_PAD": "5", "GCMX_CS_PAD": "7"},
           "padded": {"GCMX_ROW_PAD": "16", "GCMX_PLANE_PAD": "64"}}


@pytest.fixture(scope="module")
def G():
    import gcm_amd
    gcm_amd.lib()
    return gcm_amd


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {8: np.uint64, 4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = got.view(u) != want.view(u)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {at}: "
                             f"got {got[at]!r} want {want[at]!r}")


# ---------------------------------------------------------------- the cases --

def areas_for(D):
    """Overlapping areas of all four kinds.  With START and H_STD the coordinates are
    exact multiples of 0.25, and nodes lie exactly on the box's faces (x = 1.5 and
    3.0, y = -1 and 3, z = 3 and 12) and on the sphere's surface (distance exactly 2
    along an axis): strict, so outside.  Below 3-D the absent coordinates are 0.0 and
    the areas are placed to hold it."""
    if D == 3:
        return [("box", (1.5, -1.0, 3.0), (3.0, 3.0, 12.0)),
                ("sphere", 2.0, (2.5, 1.0, 8.0)),
                ("cylinder", 1.5, (2.0, 0.0, 5.0), (3.0, 2.0, 15.0))]
    if D == 2:
        return [("box", (1.5, -1.0, -1.0), (3.0, 3.0, 1.0)),
                ("sphere", 2.0, (4.5, 1.0, 0.0)),
                ("cylinder", 1.5, (5.0, 4.0, -0.5), (9.0, 30.0, 0.5))]
    return [("box", (1.5, -1.0, -1.0), (3.0, 3.0, 1.0)),
            ("sphere", 2.0, (4.5, 0.0, 0.0)),
            ("cylinder", 1.5, (8.0, -0.5, -0.25), (15.0, 0.5, 0.25))]


def vectors_for(areas, M, seed):
    rng = np.random.default_rng(seed)
    return [(a, [float(x) for x in rng.uniform(-2, 2, M)]) for a in areas]


def make_task(H, sizes, bs, model, h, start, mat_areas, vectors):
    D = len(sizes)
    t = H.Task()
    t.dimensionality = D
    t.border_size = bs
    t.h = list(h[:D])
    t.courant = 0.9
    t.number_of_snaps = 1
    t.add_body(0, list(sizes), list(start[:D]), model=model)
    t.set_default_material(4.0, 2.0, 1.0)
    for k, a in enumerate(mat_areas):
        t.add_material(a, 2.0 + k, 1.0, 1.0)
    for a, v in vectors:
        t.add_initial_vector(a, list(v))
    return t


def oracle_state(sizes, bs, h, start, mat_areas, vectors):
    D = len(sizes)
    t = O.Task(D=D, border_size=bs, h=list(h[:D]), cubics={0: (list(sizes), list(start[:D]))}, courant=0.9,
               default_material=O.Material(4.0, 2.0, 1.0),
               inhomogeneities=[(a, O.Material(2.0 + k, 1.0, 1.0)) for k, a in enumerate(mat_areas)],
               number_of_snaps=1, ic_vectors=[(a, list(v)) for a, v in vectors])
    b = O.Engine(t).bodies[0]
    return b.pde.reshape(b.shape_all + (b.M,)), b.mat_id.reshape(b.shape_all)


@functools.lru_cache(maxsize=None)
def reference(sizes, bs, model, h=H_STD):
    """host_state of the standard case on one grid, computed once per module; the
    elastic ones are compared with the oracle's set-up here."""
    from gcm_amd import _gcm_host as H
    import gcm_amd
    D = len(sizes)
    M = gcm_amd.pde_size(D, model)
    mat_areas = areas_for(D)
    vectors = vectors_for([("infinite",)] + mat_areas, M, seed=sum(sizes) + bs)
    hs = H.host_state(make_task(H, sizes, bs, model, h, START, mat_areas, vectors), 0)
    pde, ids = hs["pde"], hs["mat_ids"]
    pde.setflags(write=False)
    ids.setflags(write=False)
    if model == "elastic":
        opde, oids = oracle_state(sizes, bs, h, START, mat_areas, vectors)
        same_bits(pde, opde, f"host_state vs oracle, pde {sizes}")
        same_bits(ids, oids, f"host_state vs oracle, ids {sizes}")
    inner = ids[tuple(slice(bs, -bs) for _ in range(D))]
    assert set(np.unique(inner)) == {0, 1, 2, 3}, "every area holds some node and the default survives somewhere"
    return mat_areas, vectors, pde, ids


def layer_of(ctx):
    return ctx.download().reshape(ctx.shape_all + (ctx.M,))


def set_up(ctx, mat_areas, vectors):
    ctx.setup_state([a for a, _ in vectors], [v for _, v in vectors])
    ctx.setup_material_ids([("infinite",)] + list(mat_areas), list(range(1 + len(mat_areas))))


# ------------------------------------------------------------ context level --

@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("model", ["elastic", "acoustic"])
@pytest.mark.parametrize("sizes,bs", GRIDS)
def test_setup_equals_host_state(G, monkeypatch, sizes, bs, model, layout):
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    D = len(sizes)
    mat_areas, vectors, pde, ids = reference(tuple(sizes), bs, model)
    ctx = G.Context(D, bs, sizes, start=START[:D], h=H_STD[:D], model=model)
    before = ctx.transfer_bytes()
    set_up(ctx, mat_areas, vectors)
    same_bits(layer_of(ctx), pde, f"pde {sizes} {model} {layout}")
    same_bits(ctx.material_ids(), ids, f"ids {sizes} {model} {layout}")
    # only the small tables went to the device
    assert 0 < ctx.transfer_bytes()[1] - before[1] <= 2 * 4 * (88 + 8 * ctx.M)
    ctx.close()


def test_nodes_on_the_surfaces_are_outside():
    """What the standard case is for: the oracle's numpy restatement of contains puts
    the node on the box's face and the node on the sphere's surface outside, and
    their inner neighbours inside."""
    box, sphere, _ = areas_for(3)
    c = lambda i, j, k: tuple(np.array([float((START[d] + n)) * H_STD[d]]) for d, n in enumerate((i, j, k)))
    assert c(0, 1, 2) == (1.5, -1.0, 3.0)
    assert not O.area_contains(box, *c(0, 2, 4))[0] and not O.area_contains(box, *c(1, 1, 4))[0]
    assert not O.area_contains(box, *c(1, 2, 2))[0] and O.area_contains(box, *c(1, 2, 3))[0]
    assert c(2, 5, 22) == (2.5, 3.0, 8.0) and c(2, 3, 30) == (2.5, 1.0, 10.0)
    assert not O.area_contains(sphere, *c(2, 5, 22))[0] and not O.area_contains(sphere, *c(2, 3, 30))[0]
    assert O.area_contains(sphere, *c(2, 4, 22))[0] and O.area_contains(sphere, *c(2, 3, 29))[0]


@pytest.mark.parametrize("model", ["elastic", "acoustic"])
def test_roundings_decide_membership(G, H, model):
    """h = (0.1, 0.3, 0.7): no coordinate is exact.  A sphere off the axes whose
    radius IS the rounded distance of one node leaves that node outside, the next
    double up takes it in; the same for a cylinder's radius.  The device must put
    every node where the host does."""
    sizes, bs = [5, 7, 70], 2
    M = G.pde_size(3, model)
    xyz = [float(START[d] + n) * H_ODD[d] for d, n in enumerate((3, 4, 20))]  # CubicGrid::coords of node (3, 4, 20)
    cen = (0.47, 0.11, 20.3)
    dx, dy, dz = (np.float64(xyz[d]) - np.float64(cen[d]) for d in range(3))
    r = float(np.sqrt(dx * dx + dy * dy + dz * dz))
    b, e = (0.13, -0.57, 8.1), (0.61, 1.49, 40.7)
    axis = (np.array(e) - np.array(b))
    axis = axis / np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2])
    cb = np.array(xyz) - np.array(b)
    p = cb[0] * axis[0] + cb[1] * axis[1] + cb[2] * axis[2]
    rc = float(np.sqrt((cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2]) - p * p))
    mat_areas = [("sphere", r, cen), ("sphere", float(np.nextafter(r, np.inf)), cen),
                 ("cylinder", rc, b, e), ("cylinder", float(np.nextafter(rc, np.inf)), b, e),
                 ("cylinder", float(np.nextafter(rc, 0.0)), b, e)]
    vectors = vectors_for([("infinite",)] + mat_areas, M, seed=7)
    hs = H.host_state(make_task(H, sizes, bs, model, H_ODD, START, mat_areas, vectors), 0)
    inner = hs["mat_ids"][2:-2, 2:-2, 2:-2]
    assert len(np.unique(inner)) >= 4
    # the chosen node: outside the first sphere by its strictness, inside the second
    single = make_task(H, sizes, bs, model, H_ODD, START, mat_areas[:2], [])
    assert H.host_state(single, 0)["mat_ids"][2 + 3, 2 + 4, 2 + 20] == 2
    ctx = G.Context(3, bs, sizes, start=START, h=H_ODD, model=model)
    set_up(ctx, mat_areas, vectors)
    same_bits(layer_of(ctx), hs["pde"], f"pde {model}")
    same_bits(ctx.material_ids(), hs["mat_ids"], f"ids {model}")
    ctx.close()


def test_sum_order(G, H):
    """v = ((0.0 + 1.0) + 1e16) + -1e16 = 0.0 in the list's order; any other
    association gives 1.0."""
    sizes, bs = [3, 5, 70], 2
    vectors = [(("infinite",), [1.0] * 9), (("infinite",), [1e16] * 9), (("infinite",), [-1e16] * 9)]
    ctx = G.Context(3, bs, sizes)
    ctx.setup_state([a for a, _ in vectors], [v for _, v in vectors])
    got = layer_of(ctx)
    same_bits(got, np.zeros_like(got), "the sum in list order")
    same_bits(got, H.host_state(make_task(H, sizes, bs, "elastic", (1, 1, 1), (0, 0, 0), [], vectors), 0)["pde"],
              "host_state")
    # and the other order is seen: 1e16, -1e16, 1.0 leaves 1.0 on the inner nodes
    ctx.setup_state([a for a, _ in vectors], [vectors[1][1], vectors[2][1], vectors[0][1]])
    assert np.all(layer_of(ctx)[2:-2, 2:-2, 2:-2] == 1.0)
    ctx.close()


# ----------------------------------------------------------------- box form --

def iso_tables(D, materials):
    t = [O.isotropic_elastic_matrices(D, *m) for m in materials]
    return np.stack([x[0] for x in t]), np.stack([x[1] for x in t]), np.stack([x[2] for x in t])


def test_boxes_fill_their_nodes_only(G, H):
    """Two disjoint boxes of one context, each with its own start, as the members
    of a stack are set up: their nodes get the state of a grid of the box's extent
    that starts there; every other node keeps what it had; no ghost is written, so
    the step keeps its path."""
    sizes, bs, FILL = [6, 9, 70], 2, 3.0e300
    ctx = G.Context(3, bs, sizes, start=[0, 0, 0], h=H_ODD)
    ctx.set_materials(*iso_tables(3, [(4.0, 2.0, 1.0)]))
    state = np.zeros(ctx.shape_all + (9,))
    state[2:-2, 2:-2, 2:-2] = FILL
    ctx.upload(state)
    path = ctx.effective_path
    assert path == "fused"
    boxes = [((0, 0, 0), (6, 4, 70), (3, -2, 10)), ((1, 5, 3), (5, 9, 68), (-7, 40, 1))]
    want, want_ids = state.copy(), np.zeros(ctx.shape_all, dtype=np.uint8)
    ids_calls = []
    for k, (lo, hi, start) in enumerate(boxes):
        ext = [b - a for a, b in zip(lo, hi)]
        cen = tuple(float(start[d] + ext[d] // 2) * H_ODD[d] for d in range(3))
        areas = [("infinite",), ("sphere", 0.45, cen), ("cylinder", 0.4, cen, (cen[0] + 0.2, cen[1] + 0.9, cen[2] + 9.0))]
        vectors = vectors_for(areas, 9, seed=k)
        mats = [("sphere", 0.5, cen)]
        hs = H.host_state(make_task(H, ext, bs, "elastic", H_ODD, start, mats, vectors), 0)
        sl = tuple(slice(bs + a, bs + b) for a, b in zip(lo, hi))
        want[sl] = hs["pde"][2:-2, 2:-2, 2:-2]
        want_ids[sl] = hs["mat_ids"][2:-2, 2:-2, 2:-2]
        assert np.any(hs["mat_ids"] == 1) and len(np.unique(hs["pde"])) > 3
        ctx.setup_state(areas, [v for _, v in vectors], box=(lo, hi, start))
        ids_calls.append(([("infinite",)] + mats, [0, 1], (lo, hi, start)))
    same_bits(layer_of(ctx), want, "two boxes")
    assert (want == FILL).sum() > 0
    # no node list and no contact copy is needed after it: the step's path is what it was
    assert ctx.effective_path == path
    ctx.set_materials(*iso_tables(3, [(4.0, 2.0, 1.0), (2.0, 1.0, 1.0)]))
    for areas, id_of, box in ids_calls:
        ctx.setup_material_ids(areas, id_of, box=box)
    same_bits(ctx.material_ids(), want_ids, "two boxes, ids")
    same_bits(layer_of(ctx), want, "two boxes, after the ids")
    ctx.close()


# ------------------------------------------------------------------- census --

def test_census_is_exact(G, H):
    sizes, bs = [5, 7, 70], 2
    box, sphere, cyl = areas_for(3)
    far = ("sphere", 1.0, (100.0, 100.0, 100.0))  # holds no node
    ctx = G.Context(3, bs, sizes, start=START, h=H_STD)
    before = layer_of(ctx).copy()

    def host_ids(mat_areas):
        ids = H.host_state(make_task(H, sizes, bs, "elastic", H_STD, START, mat_areas, []), 0)["mat_ids"]
        return np.unique(ids[2:-2, 2:-2, 2:-2])

    for mat_areas in ([box, sphere, cyl], [box, far, sphere], [far], [box, ("infinite",), sphere],
                      [("infinite",)], [box, sphere, ("infinite",)]):
        areas = [("infinite",)] + mat_areas
        got = ctx.setup_census(areas, list(range(len(areas))))
        assert list(got) == list(host_ids(mat_areas)), mat_areas
    # a default entirely hidden by a later infinite area is unused; so is all before it
    assert list(ctx.setup_census([("infinite",), box, ("infinite",), sphere], [0, 1, 2, 3])) == [2, 3]
    # the mask is of id_of's values, wherever they lie in 0..255, and of the box asked for
    assert list(ctx.setup_census([("infinite",), box, sphere], [200, 31, 32])) == [31, 32, 200]
    assert list(ctx.setup_census([("infinite",), box], [9, 64], box=((3, 0, 0), (5, 7, 70), (6, -2, 10)))) == [9]
    # nothing was written, and no id array exists
    same_bits(layer_of(ctx), before, "the layer after the census")
    assert not ctx.material_ids().any()
    ctx.close()


def hidden_default_task(H, flag):
    t = make_task(H, [8, 9, 64], 2, "elastic", (1, 1, 1), (0, 0, 0), [("infinite",)],
                  [(("sphere", 3.0, (4.0, 4.0, 32.0)), [0.0] * 3 + [-1.0, 0, 0, -1.0, 0, -1.0])])
    t.set_device_setup(flag)
    return t


def test_engine_hidden_default_stays_homogeneous(H):
    """The default material entirely under a later infinite area: one material is
    used, no id array, the homogeneous kernels -- with the flag as without."""
    seen = []
    for flag in (False, True):
        e = H.Engine(hidden_default_task(H, flag))
        ms, path = e.matrix_structure(0), e.path(0)
        e.run_steps(1)
        seen.append((ms, path, e.last_path(0), e.pde(0).tobytes()))
    assert seen[0][:3] == seen[1][:3] and seen[0][0] == 1
    assert seen[0][3] == seen[1][3]


# ------------------------------------------------------------------- errors --

def test_refusals_change_nothing(G):
    sizes, bs = [5, 7, 70], 2
    mat_areas, vectors, pde, ids = reference(tuple(sizes), bs, "elastic")
    ctx = G.Context(3, bs, sizes, start=START, h=H_STD)
    ctx.set_materials(*iso_tables(3, [(4.0, 2.0, 1.0), (2.0, 1.0, 1.0), (3.0, 1.0, 1.0), (4.0, 1.0, 1.0)]))
    set_up(ctx, mat_areas, vectors)
    path = ctx.effective_path
    gx = G.gcmx
    inf = ("infinite",)
    bad_kind = gx.Area()
    bad_kind.kind = 7
    nan_sphere = ("sphere", 1.0, (float("nan"), 0.0, 0.0))
    inf_box = ("box", (-float("inf"), 0.0, 0.0), (1.0, 1.0, 1.0))
    bad_area_lists = [[], [inf] * 257, [bad_kind], [inf, nan_sphere], [inf_box], [("sphere", 0.0, (1.0, 1.0, 1.0))],
                      [("sphere", -1.0, (1.0, 1.0, 1.0))], [("cylinder", 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))],
                      [("cylinder", 1.0, (0.0, 0.0, float("inf")), (1.0, 1.0, 1.0))],
                      [("box", (0.0, 0.0, 0.0), (1.0, 0.0, 1.0))], [("box", (0.0, 2.0, 0.0), (1.0, 1.0, 1.0))]]
    bad_boxes = [((1, 1, 1), (1, 3, 3), START), ((2, 1, 1), (1, 3, 3), START), ((0, 0, 0), (5, 7, 71), START),
                 ((-1, 0, 0), (5, 7, 70), START), ((0, 0, 0), (6, 7, 70), START)]

    def refused(call, what):
        with pytest.raises(G.GcmxError) as e:
            call()
        assert e.value.status == ERR_INVALID_ARG, what

    for areas in bad_area_lists:
        n = len(areas)
        refused(lambda: ctx.setup_state(areas, np.ones((n, 9))), ("state", areas))
        refused(lambda: ctx.setup_census(areas, [0] * n), ("census", areas))
        refused(lambda: ctx.setup_material_ids(areas, [0] * n), ("ids", areas))
    for box in bad_boxes:
        refused(lambda: ctx.setup_state([inf], np.ones((1, 9)), box=box), ("state", box))
        refused(lambda: ctx.setup_census([inf], [0], box=box), ("census", box))
        refused(lambda: ctx.setup_material_ids([inf], [0], box=box), ("ids", box))
    refused(lambda: ctx.setup_material_ids([inf, inf], [0, 4]), "an id the four materials do not have")
    # null pointers, through the library itself
    lib = G.lib()
    one = (gx.Area * 1)(gx.make_area(inf))
    vec = (ctypes.c_double * 9)()
    idb = (ctypes.c_uint8 * 1)(0)
    used = (ctypes.c_uint32 * 8)()
    for what, status in {
            "state, areas": lib.gcmx_setup_state(ctx.ptr, None, 1, None, vec),
            "state, vectors": lib.gcmx_setup_state(ctx.ptr, None, 1, one, None),
            "census, areas": lib.gcmx_setup_census(ctx.ptr, None, 1, None, idb, used),
            "census, id_of": lib.gcmx_setup_census(ctx.ptr, None, 1, one, None, used),
            "census, used": lib.gcmx_setup_census(ctx.ptr, None, 1, one, idb, None),
            "ids, areas": lib.gcmx_setup_material_ids(ctx.ptr, None, 1, None, idb),
            "ids, id_of": lib.gcmx_setup_material_ids(ctx.ptr, None, 1, one, None),
            "download": lib.gcmx_download_material_ids(ctx.ptr, None)}.items():
        assert status == ERR_INVALID_ARG, what
    same_bits(layer_of(ctx), pde, "the layer after the refusals")
    same_bits(ctx.material_ids(), ids, "the ids after the refusals")
    assert ctx.effective_path == path
    ctx.close()


# ------------------------------------------------------------------- engine --

def cube_task(H):
    from tests.taskspec import host_task, spec
    N = 12
    s = spec(3, 2, [1, 1, 1], {0: ([N] * 3, [0] * 3)}, 0.9, (4, 2, 1), snaps=3, steps_per_snap=2,
             quantities=[(("sphere", 3.0, (6.0, 6.0, 6.0)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_vtk_quantities(["PRESSURE"])
    return t, [0]


def stack_task(H):
    """Two bodies stacked along y; the upper part of the second is another material."""
    from tests.taskspec import host_task, spec
    X, Y, Z = 10, 12, 64
    cubics = {0: ([X, 5, Z], [0, 0, 0]), 1: ([X, 7, Z], [0, 5, 0])}
    s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=2, steps_per_snap=2,
             quantities=[(("sphere", 5.0, (X / 2, 3.5, Z / 2)), "PRESSURE", 10.0)],
             waves=[(("box", (-1, -1, 10.5), (100, 100, 20.5)), "P_FORWARD", 2, "Vz", -2.0)])
    t = host_task(s)
    t.add_material(("box", (-1, 8.5, -1), (100, 100, 100)), 2, 1, 1, number=5)
    t.set_vtk_quantities(["PRESSURE", "Vy"])
    return t, [0, 1]


def stack_same_material_task(H):
    """The same stack with a second condition of the SAME material (another
    material number) in the second member: the stack's table shares the entry, the
    device ids cannot tell the two conditions apart, the files' material array must."""
    t, bodies = stack_task(H)
    t.add_material(("sphere", 3.0, (5.0, 9.0, 32.0)), 2, 1, 1, number=9)
    return t, bodies


def ortho_layers_task(H):
    """One orthotropic body of three layers along x."""
    from tests.test_ortho_cpu import MAT_A, MAT_B
    from tests.test_ortho_het_cpu import hand_permutation
    t = H.Task()
    t.dimensionality = 3
    t.border_size = 2
    t.h = [1.0, 1.0, 1.0]
    t.courant = 0.9
    t.add_body(0, [12, 9, 64], [0, 0, 0])
    t.set_default_orthotropic_material(MAT_B[0], list(MAT_B[1]), number=1)
    t.add_orthotropic_material(("box", (3.5, -1, -1), (7.5, 100, 100)), MAT_B[0], list(hand_permutation(MAT_B[1])), number=2)
    t.add_orthotropic_material(("box", (7.5, -1, -1), (100, 100, 100)), MAT_A[0], list(MAT_A[1]), number=3)
    t.add_initial_quantity(("sphere", 4.0, (6.0, 4.5, 32.0)), "PRESSURE", 10.0)
    t.set_vtk_quantities(["PRESSURE", "Sxy"])
    return t, [0]


def acoustic_task(H):
    """The 2-D acoustic launcher task (launcher/main.cpp:422-467)."""
    t = H.Task()
    t.dimensionality = 2
    t.border_size = 2
    t.h = [1.0, 1.0]
    t.courant = 1.0
    t.add_body(0, [40, 30], [0, 0], model="acoustic")
    t.set_default_material(1.0, 1.0, 0.0)
    t.add_initial_quantity(("sphere", 6.0, (20.0, 15.0, 0.0)), "PRESSURE", 10.0)
    t.add_border_condition(0, 1, ("box", (-1e3, -1e3, -1e3), (1e3, 1e-5, 1e3)), {"PRESSURE": lambda time: 0.0})
    t.set_vtk_quantities(["PRESSURE", "Vx"])
    return t, [0]


def xcontact_task(H):
    """Two bodies in contact along x, run as separate bodies (GCMX_NO_STACKS=1)."""
    from tests.taskspec import host_task, spec
    X, Y, Z = 12, 20, 64
    cubics = {0: ([X, Y, Z], [0, 0, 0]), 1: ([X, Y, Z], [X, 0, 0])}
    s = spec(3, 2, [1, 1, 1], cubics, 0.9, (4, 2, 1), snaps=6,
             quantities=[(("sphere", 6.0, (X - 1.5, Y / 2, Z / 2)), "PRESSURE", 10.0)])
    t = host_task(s)
    t.set_vtk_quantities(["PRESSURE"])
    return t, [0, 1]


def run_engine(H, make, flag, out):
    t, bodies = make(H)
    t.set_device_setup(flag)
    t.add_snapshotter("VTK")
    t.output_directory = out
    t.number_of_snaps = 3
    t.steps_per_snap = 1
    e = H.Engine(t)
    res = {"h2d": {i: e.transfer_bytes(i)[1] for i in bodies}, "pde0": {i: e.pde(i) for i in bodies}}
    e.run()
    assert e.steps == 3
    res["pde3"] = {i: e.pde(i) for i in bodies}
    res["path"] = {i: e.last_path(i) for i in bodies}
    res["files"] = {(i, s): open(f"snapshots/{out}/vtk/mesh{i}core00snap{s:04d}.vts", "rb").read()
                    for i in bodies for s in range(4)}
    return res


@pytest.mark.parametrize("make", [cube_task, stack_task, stack_same_material_task, ortho_layers_task, acoustic_task,
                                  xcontact_task])
def test_engine_device_setup_equals_host_setup(H, tmp_path, monkeypatch, make):
    monkeypatch.chdir(tmp_path)
    if make is xcontact_task:
        monkeypatch.setenv("GCMX_NO_STACKS", "1")
    off, on = run_engine(H, make, False, "off"), run_engine(H, make, True, "on")
    for i in off["pde0"]:
        same_bits(on["pde0"][i], off["pde0"][i], f"{make.__name__} body {i} after set-up")
        same_bits(on["pde3"][i], off["pde3"][i], f"{make.__name__} body {i} after 3 steps")
        assert on["path"][i] == off["path"][i]
        layer = off["pde0"][i].size * 8
        assert off["h2d"][i] >= layer
        assert on["h2d"][i] < layer // 8, (on["h2d"][i], layer)
    assert any(np.any(p != 0) for p in off["pde0"].values())
    assert off["files"].keys() == on["files"].keys()
    for key in off["files"]:
        assert off["files"][key] == on["files"][key], (make.__name__, key)
    # the material array of the files is not a constant where the body has several materials
    from tests.helpers import read_vts
    for body, n_materials in {stack_task: [(1, 2)], stack_same_material_task: [(1, 3)], ortho_layers_task: [(0, 3)]}.get(make, []):
        arrays = read_vts(str(tmp_path / f"snapshots/on/vtk/mesh{body}core00snap0000.vts"))[1]
        assert len(np.unique(arrays["material_index"])) == n_materials
