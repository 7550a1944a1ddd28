"""k_trace2's box test on the global-memory, non-quantised instances: each axis's near and far
plane is loaded by the sign of the ray's inverse direction (slab_rule.h), a leaf lane's six floats
by 16-B loads at 4-B steps, and the two products of an axis are not sorted. Rays the rule is not
exact for (a zero, infinite or NaN component) and trees with a NaN or an inverted bound run the
scalar twin.

Each render is 40 x 30 pixels at 2 spp, in both accumulation modes, against the CPU oracle on the
same tree: image bit for bit and counters equal (assert_parity), which is what catches a box test
that passes too often. The 102-primitive grid's tree is past the LDS limit, so it runs the
instance C3 runs; IZPI_TUNE_NO_LEAF_SHORTCUT re-tests every leaf, so every leaf lane loads its
record by sign, the array's last record included.
"""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer
from izpi_amd.scene import HostScene
from oracle import oracle as O
from tests.table_cases import log_line
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_trace_addressing import grid_scene
from tests.test_gpu_trace_leaf_sizes import spheres_scene
from tests.test_oracle_kats import formula_cases

W, H, SPP = 40, 30, 2
ACCS = pytest.mark.parametrize("acc", [N.ACC_FORWARD, N.ACC_RECURSIVE], ids=["forward", "recursive"])
NODE = np.dtype([("b", "<f4", (6, 4)), ("child", "<i4", 4), ("pc", "<i4", 4)])
F32_MAX = np.float32(3.4028234663852886e38)
fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

_SCENES = {}
_TREES = {}
_REFS = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = {"grid": lambda: grid_scene(False), "box": configs.cornell_rgb, "spheres": lambda: spheres_scene(False),
                         "dragon": lambda: configs.cornell_dragon(1.0, n=40)}[name]()
    return _SCENES[name]


def lbvh_tree(name):
    """The linear BVH4 over scene `name` with at most 3 primitives per leaf: (nodes, order)."""
    if name not in _TREES:
        h = HostScene(scene_of(name), aspect_override=W / H, skip_bvh=True)
        _TREES[name] = O.lbvh4(h.prim_boxes(), 3)
        h.close()
    nodes, order = _TREES[name]
    return nodes.copy(), order.copy()


def oracle_ref(key, name, acc, tree):
    """The oracle's canvas and counters of scene `name` on `tree` ((nodes, order), or None for the
    reference builder's), computed once per key and accumulation mode."""
    if (key, acc) not in _REFS:
        o = O.OracleScene(scene_of(name), aspect_override=W / H)
        if tree is not None:
            o.set_bvh(*tree)
        req = N.RenderReq(width=W, height=H, spp=SPP, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        ref, stats = o.render(req, threads=16)
        o.close()
        _REFS[(key, acc)] = (ref.reshape(H, W, 4), stats, None if tree is None else tree[0].tobytes())
    return _REFS[(key, acc)]


def render_and_compare(name, acc, capfd, flags=0, bvh="reference", host=None, key=None, tree=None):
    """Render `name` (on the GPU-built tree of 3-primitive leaves, the reference tree, or `host`'s
    tree `tree`), compare with the oracle on that tree, and return the pass log's lines."""
    kw = dict(host_scene=host) if host is not None else dict(bvh=bvh, bvh_leaf_max=3 if bvh == "gpu" else None)
    r = GPURenderer(scene_of(name), W, H, SPP, tuning=N.tuning(flags=flags | N.TUNE_PASS_LOG), accumulation=acc, **kw)
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    if bvh == "gpu" and host is None:
        tree = (r.bvh_nodes(), r.host._bvh_keep[1])
    ref, ostats, tree_bytes = oracle_ref(key or (name, bvh), name, acc, tree)
    if tree is not None:
        assert tree[0].tobytes() == tree_bytes  # the same tree every time
    assert_parity(img, ref, r.stats, ostats)
    stats = dict(r.stats)
    r.close()
    return log_line(err, "IZPI_TRACE_INSTANCE"), log_line(err, "IZPI_TRACE_ADDR"), stats


GRID_FLAGS = [0, N.TUNE_NO_LEAF_SHORTCUT, N.TUNE_WIDE_ADDR, N.TUNE_NO_RAY_LDS, N.TUNE_SCALAR_SLAB]


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("bvh", ["gpu", "reference"])
@pytest.mark.parametrize("flags", GRID_FLAGS, ids=["plain", "no_leaf_shortcut", "wide_addr", "no_ray_lds", "scalar_slab"])
def test_grid_bitwise(gpu, capfd, acc, bvh, flags):
    trace, addr, stats = render_and_compare("grid", acc, capfd, flags, bvh)
    assert (trace["lds_bvh"], trace["q"], trace["tri"]) == (0, 0, 1), trace
    assert trace["ray_lds"] == int(not flags & N.TUNE_NO_RAY_LDS) and addr["a32"] == int(not flags & N.TUNE_WIDE_ADDR), (trace, addr)
    assert stats["node_steps"] > 0 and stats["prim_steps"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", [N.TUNE_NO_LDS_BVH, N.TUNE_NO_LDS_BVH | N.TUNE_NO_LEAF_SHORTCUT], ids=["global_tree", "no_leaf_shortcut"])
def test_cornell_box_from_global_memory_bitwise(gpu, capfd, acc, flags):
    """The Cornell box alone, its tree read from global memory instead of LDS."""
    trace, _, stats = render_and_compare("box", acc, capfd, flags)
    assert (trace["lds_bvh"], trace["q"]) == (0, 0), trace
    assert stats["node_steps"] > 0


SPHERE_FLAGS = [0, N.TUNE_WIDE_ADDR, N.TUNE_NO_DIST, N.TUNE_NO_DIST | N.TUNE_WIDE_ADDR]


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", SPHERE_FLAGS, ids=["dist", "dist_wide", "one_per_lane", "one_per_lane_wide"])
def test_sphere_capable_instances_bitwise(gpu, capfd, acc, flags):
    """The Cornell box with three spheres, its tree read from global memory: the sphere-capable
    instances carry the three near-plane indices packed in one register; the one-ray-per-lane
    instance on 64-bit addresses keeps the planes in order (slab4_fast)."""
    trace, addr, stats = render_and_compare("spheres", acc, capfd, flags | N.TUNE_NO_LDS_BVH)
    assert (trace["lds_bvh"], trace["q"], trace["tri"]) == (0, 0, 0), trace
    assert trace["dist"] == int(not flags & N.TUNE_NO_DIST) and addr["a32"] == int(not flags & N.TUNE_WIDE_ADDR), (trace, addr)
    assert stats["node_steps"] > 0 and stats["sph_tests"] > 0


def user_tree(kind):
    """The grid's linear BVH4 with one node changed: `empty_hit`, an empty slot (child -1) whose
    box every ray hits; `inverted`, a valid slot of an inner node with its x bounds swapped."""
    nodes, order = lbvh_tree("grid")
    rec = nodes.view(NODE).reshape(-1)
    inner = [k for k in range(len(rec)) if rec[k]["pc"][0] == 0]
    if kind == "empty_hit":
        k, i = next((k, i) for k in inner for i in range(4) if rec[k]["child"][i] == -1)
        rec[k]["b"][:3, i] = -1e30
        rec[k]["b"][3:, i] = 1e30
    else:
        k, i = next((k, i) for k in inner for i in range(4) if rec[k]["child"][i] != -1 and rec[k]["b"][0, i] < rec[k]["b"][3, i])
        rec[k]["b"][0, i], rec[k]["b"][3, i] = rec[k]["b"][3, i], rec[k]["b"][0, i]
    return nodes, order


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("kind", ["empty_hit", "inverted"])
def test_user_tree_bitwise(gpu, capfd, acc, kind):
    """A tree from izpi_host_scene_set_bvh with an empty slot every ray's box test passes (its
    child stays unvisited), and one with an inverted valid slot (ordered_bounds is 0: every ray
    runs the twin, whose swap reads the box as the oracle does)."""
    tree = user_tree(kind)
    host = HostScene(scene_of("grid"), aspect_override=W / H, skip_bvh=True)
    host.set_bvh(*tree)
    trace, _, stats = render_and_compare("grid", acc, capfd, host=host, key=("grid", kind), tree=tree)
    assert (trace["lds_bvh"], trace["q"]) == (0, 0), trace
    assert stats["node_steps"] > 0 and stats["prim_steps"] > 0


def explicit_rays(nodes, n=4096, seed=11):
    """n rays [o, d, tMin, tMax], each through a random point of the root's box: the 8 sign octants
    evenly; every 5th ray with one direction component exactly 0 (its inverse is infinite: the lane
    is not fast, so waves mix fast and other lanes); every 7th ray with an origin component set to
    an f32 bound of a node; every 11th ray with a negative tMin (accepted hits behind the origin
    make its running tMax negative)."""
    rng = np.random.default_rng(seed)
    rec = nodes.view(NODE).reshape(-1)
    valid = rec[0]["child"] != -1
    lo, hi = rec[0]["b"][:3, valid].min(1).astype(np.float64), rec[0]["b"][3:, valid].max(1).astype(np.float64)
    bounds = rec["b"].reshape(-1)
    bounds = bounds[np.abs(bounds) < 1e6].astype(np.float64)
    sign = np.stack([np.where((np.arange(n) >> a) & 1, -1.0, 1.0) for a in range(3)], 1)
    d = sign * (np.abs(rng.normal(size=(n, 3))) + 1e-3)
    target = rng.uniform(lo, hi, (n, 3))
    rays = np.zeros((n, 8))
    rays[:, :3] = target - d * rng.uniform(5.0, 60.0, (n, 1))
    zero = np.arange(0, n, 5)
    d[zero, zero % 3] = 0.0
    rays[:, 3:6] = d
    on = np.arange(0, n, 7)
    rays[on, on % 3] = bounds[rng.integers(0, len(bounds), len(on))]
    rays[:, 6], rays[:, 7] = 0.001, np.finfo(np.float64).max
    rays[::11, 6] = -0.5
    return rays, sign


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid", "dragon"])
def test_explicit_rays_bitwise(gpu, name):
    """izpi_gpu_trace (per-entry tMin and tMax) against OracleScene.trace: the hit records' first
    72 bytes, as test_trace_closest_hit_bitwise compares them."""
    scene = scene_of(name)
    r = GPURenderer(scene, 16, 16, 1)
    o = O.OracleScene(scene, aspect_override=1.0)
    rays, sign = explicit_rays(r.bvh_nodes())
    octant = (sign[:, 0] < 0) * 1 + (sign[:, 1] < 0) * 2 + (sign[:, 2] < 0) * 4
    assert list(np.bincount(octant, minlength=8)) == [len(rays) // 8] * 8
    got = (N.Hit * len(rays))()
    assert N.lib().izpi_gpu_trace(r.ctx, rays.ctypes.data_as(C.POINTER(C.c_double)), len(rays), got) == 0
    want = o.trace(rays)
    hits = 0
    for i in range(len(rays)):
        g, w = got[i], want[i]
        assert g.hit == w.hit, i
        if w.hit:
            hits += 1
            assert g.prim_ref == w.prim_ref, i
            assert bytes(g)[:72] == bytes(w)[:72], (i, g.t, w.t)
    assert len(rays) // 8 < hits < len(rays)  # (rays through the root's box: a good part hits, some miss)
    o.close()
    r.close()


def slab_pairs():
    """(boxes [n][24], rays [n][7]): the reference KATs, the 1000 formula cases, and 8 octants x 512
    random pairs whose slots are, in turn, plain boxes, flat boxes, boxes with the origin on a
    plane, boxes behind the ray, huge and infinite bounds, subnormal extents, and (every 16th pair)
    a negative or NaN tMax, or a box or ray the sorted rule is not exact for, so that waves mix the
    two paths."""
    kats = json.loads((Path(__file__).parent / "golden" / "reference_kats.json").read_text())["ray_aabb4"]
    f = lambda v: [float("inf") if x == "inf" else float(x) for x in v]
    kb = [f(c["min_x"]) + f(c["min_y"]) + f(c["min_z"]) + f(c["max_x"]) + f(c["max_y"]) + f(c["max_z"]) for c in kats]
    kr = [f(c["org"]) + f(c["invdir"]) + [float(c["tmax"])] for c in kats]
    fb, fr = formula_cases()
    rng = np.random.default_rng(18)
    n = 8 * 512
    o = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    d = rng.uniform(1e-3, 1.0, (n, 3))
    d[rng.random((n, 3)) < 0.05] = 1e-30  # products overflow
    for a in range(3):
        d[:, a] *= np.where(((np.arange(n) // 512) >> a) & 1, -1.0, 1.0)
    inv = (1.0 / d).astype(np.float32)
    tmax = rng.choice(np.array([np.inf, 0.0, 1e-30, 1e-42, 5.0, 60.0, 1e4], np.float32), n)
    c = rng.uniform(-60, 60, (n, 3, 4)).astype(np.float32)
    h = rng.uniform(0, 30, (n, 3, 4)).astype(np.float32)
    kind = rng.integers(0, 8, (n, 1, 4))
    h = np.where(kind == 1, np.float32(0), h)                                       # flat
    h = np.where(kind == 5, np.float32(1e-41), h)                                   # subnormal extent
    mn, mx = c - h, c + h
    mn = np.where(kind == 2, o[:, :, None], mn)                                     # origin on the min plane
    mx = np.where(kind == 3, o[:, :, None], mx)                                     # ... on the max plane
    mn, mx = np.minimum(mn, mx), np.maximum(mn, mx)
    mn = np.where(kind == 4, -F32_MAX, mn); mx = np.where(kind == 4, F32_MAX, mx)   # huge
    mn = np.where(kind == 6, np.float32(-np.inf), mn); mx = np.where(kind == 6, np.float32(np.inf), mx)  # infinite
    behind = (kind == 7)                                                            # wholly behind the ray
    sgn = np.sign(inv)[:, :, None]
    mn = np.where(behind, np.where(sgn > 0, o[:, :, None] - 40, o[:, :, None] + 10), mn)
    mx = np.where(behind, np.where(sgn > 0, o[:, :, None] - 10, o[:, :, None] + 40), mx)
    boxes = np.concatenate([mn.reshape(n, 12), mx.reshape(n, 12)], 1).astype(np.float32)
    rays = np.concatenate([o, inv, tmax[:, None]], 1).astype(np.float32)
    odd = np.arange(3, n, 16)
    for j, i in enumerate(odd):
        what = j % 6
        if what == 0: rays[i, 3 + j % 3] = np.inf
        elif what == 1: rays[i, 3 + j % 3] = 0.0
        elif what == 2: rays[i, 6] = -1.0
        elif what == 3: rays[i, 6] = np.nan
        elif what == 4: boxes[i, j % 12] = np.nan
        else: boxes[i, [0, 12]] = boxes[i, [12, 0]] + np.float32([1.0, 0.0])          # slot 0 inverted on x
    return (np.concatenate([np.array(kb, np.float32), fb, boxes]), np.concatenate([np.array(kr, np.float32), fr, rays]),
            [c["expected"] for c in kats])


@pytest.mark.gpu
def test_debug_slab4_equals_oracle_and_twin(gpu):
    """izpi_gpu_debug_slab4 (the kernel's near-index rule, plane selection and sorted test, in
    whole waves) against oracle_ray_aabb4 and against izpi_gpu_ray_aabb4, the scalar twin."""
    boxes, rays, kat_expected = slab_pairs()
    boxes, rays = np.ascontiguousarray(boxes), np.ascontiguousarray(rays)
    with np.errstate(all="ignore"):
        want = np.array([O.lib().oracle_ray_aabb4(fptr(b), fptr(r)) for b, r in zip(boxes, rays)], np.uint8)
    assert list(want[:len(kat_expected)]) == kat_expected
    assert 0 < np.count_nonzero(want[-4096:]) < 4096 and len({int(m) for m in want[-4096:]}) == 16
    r = GPURenderer(configs.cornell_rgb(), 8, 8, 1)
    for n in (len(boxes), 1, 63, 65, 1000):  # whole waves: lanes past n take no part in the result
        sorted_, twin = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
        assert N.lib().izpi_gpu_debug_slab4(r.ctx, fptr(boxes[-n:]), fptr(rays[-n:]), n, sorted_.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        assert N.lib().izpi_gpu_ray_aabb4(r.ctx, fptr(boxes[-n:]), fptr(rays[-n:]), n, twin.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        np.testing.assert_array_equal(twin, want[-n:])
        np.testing.assert_array_equal(sorted_, want[-n:])
    r.close()
