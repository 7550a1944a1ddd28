"""k_trace2's distributed primitive step in its two sizes, and its tMin in its two forms.

Where no leaf of the uploaded tree holds more than three primitives (DevScene::leaf_max, what the
GPU builder's trees have) the step sums two bits of the leaf sizes and writes, reads back and
accepts three entries per leaf; other trees, and IZPI_TUNE_LEAF4, run the form for four. Where
the scene has no dielectric and the launch no per-entry bounds, tMin is the constant 0.001 and
the step fetches neither the owner's kind word nor its entry; a glass scene runs the explicit
form. The wave masks that replaced the per-lane `advance`, `in primitive mode` and shortcut
flags are in every instance, so every case below checks them too: node visits, which include
the shortcut visits counted from those masks, must equal the oracle's.

Each render is 40 x 30 pixels at 2 spp, in both accumulation modes, against the CPU oracle on the
same tree: image bit for bit and counters equal (assert_parity). Trees with a chosen largest
leaf are the oracle's restatement of the GPU builder (oracle.lbvh4, bit for bit the device
builder's: tests/test_bvh_build.py), attached to the host scene and to the oracle alike.

At 40 x 30 x 2 a wave never holds more than 16 rays: k_trace2 shrinks its chunks to spread a short
queue over all resident waves (at least 16 entries each), so 16 lanes x 4 primitives fill a batch
of 64 exactly and no lane is left unserved. The one case that needs waves with more than 64 pending
tests therefore renders 320 x 256 x 2 (164k camera rays: 32 per wave on 5120 resident waves, more
on a smaller device), the smallest round size at which a batch overflows with three primitives
per leaf as well (22 lanes).
"""
import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer
from izpi_amd.scene import HostScene
from oracle import oracle as O
from tests.table_cases import log_line
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_trace_addressing import grid_scene, nested_chain_scene, one_triangle_scene
from tests.test_gpu_trace_steps import centre_ray_stack_depth

W, H, SPP = 40, 30, 2
BIG = (320, 256, 2)
ACCS = pytest.mark.parametrize("acc", [N.ACC_FORWARD, N.ACC_RECURSIVE], ids=["forward", "recursive"])
NODE = np.dtype([("b", "<f4", (6, 4)), ("child", "<i4", 4), ("pc", "<i4", 4)])

_SCENES = {}
_TREES = {}
_REFS = {}


def fan_scene(n=61):
    """n large blades round the camera's axis at slightly different depths, each spanning the
    view, under a two-triangle light: every camera ray meets many overlapping leaves at once, so
    most of a wave's lanes scan a leaf in the same step."""
    s = configs.Scene("fan")
    light = s.diffuse_light(emit=s.constant((4.0, 3.5, 3.0)))
    mat = s.lambert(albedo=s.constant((0.6, 0.7, 0.5)))
    k = np.arange(n)
    a = 2 * np.pi * k / n
    z = 20.0 + 0.5 * k
    v0 = np.stack([50 + 70 * np.cos(a), 50 + 70 * np.sin(a), z], -1)
    v1 = np.stack([50 + 70 * np.cos(a + 2.4), 50 + 70 * np.sin(a + 2.4), z + 0.3], -1)
    v2 = np.stack([50 + 70 * np.cos(a + 4.2), 50 + 70 * np.sin(a + 4.2), z + 0.1], -1)
    s.add_triangles(configs.f32(v0), configs.f32(v1), configs.f32(v2), mat)
    s.add_triangles([(20, 99, 20), (20, 99, 20)], [(80, 99, 20), (80, 99, 35)], [(80, 99, 35), (20, 99, 35)], light)
    configs.cornell_camera(s, W / H)
    return s


def glass_pane_scene():
    """The Cornell box with a tilted glass pane of 40 triangles in it: triangles only, but the
    dielectric makes path-length rays (tMin 0, tMax 1000), so tMin is per ray."""
    s = configs.Scene("glass_pane")
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    glass = s.dielectric(ref_idx=1.5)
    v0, v1, v2 = [], [], []
    for i in range(20):
        x0, x1 = 20.0 + 3.0 * i, 23.0 + 3.0 * i
        a, b, c, d = (x0, 15.0, 40.0 + 0.4 * i), (x1, 15.0, 40.4 + 0.4 * i), (x1, 80.0, 48.4 + 0.4 * i), (x0, 80.0, 48.0 + 0.4 * i)
        v0 += [a, a]; v1 += [b, c]; v2 += [c, d]
    s.add_triangles(v0, v1, v2, glass)
    configs.cornell_camera(s, W / H)
    return s


def spheres_scene(glass):
    """The Cornell box with three spheres (static): leaves hold spheres and triangles, so the
    owners accept through the loop that knows both. glass: one sphere is a dielectric."""
    s = configs.Scene("spheres_glass" if glass else "spheres")
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    s.add_sphere((30.0, 18.0, 45.0), 18.0, mats["White"])
    s.add_sphere((68.0, 14.0, 30.0), 14.0, s.dielectric(ref_idx=1.5) if glass else mats["Green"])
    s.add_sphere((55.0, 40.0, 70.0), 12.0, mats["Red"])
    configs.cornell_camera(s, W / H)
    return s


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = {"one": one_triangle_scene, "grid": lambda: grid_scene(False), "fan": fan_scene, "chain": nested_chain_scene,
                         "glass_pane": glass_pane_scene, "spheres": lambda: spheres_scene(False),
                         "spheres_glass": lambda: spheres_scene(True)}[name]()
    return _SCENES[name]


def tree_of(name, leaf_max):
    """(nodes, order) of the linear BVH4 over scene `name` with at most leaf_max primitives per
    leaf, or None for the reference builder's tree (leaf_max None)."""
    if leaf_max is None:
        return None
    if (name, leaf_max) not in _TREES:
        h = HostScene(scene_of(name), aspect_override=W / H, skip_bvh=True)
        _TREES[(name, leaf_max)] = O.lbvh4(h.prim_boxes(), leaf_max)
        h.close()
    return _TREES[(name, leaf_max)]


def host_of(name, leaf_max, aspect):
    tree = tree_of(name, leaf_max)
    h = HostScene(scene_of(name), aspect_override=aspect, skip_bvh=tree is not None)
    if tree is not None:
        h.set_bvh(*tree)
    return h


def leaf_sizes(host):
    pc = np.frombuffer(host.nodes().tobytes(), dtype=NODE)["pc"][:, 0]
    return sorted(set(int(c) for c in pc[pc > 0]))


def oracle_ref(name, leaf_max, acc, size):
    """The oracle's canvas and counters, computed once per scene, tree, mode and size."""
    key = (name, leaf_max, acc, size)
    if key not in _REFS:
        w, h, spp = size
        o = O.OracleScene(scene_of(name), aspect_override=w / h)
        tree = tree_of(name, leaf_max)
        if tree is not None:
            o.set_bvh(*tree)
        req = N.RenderReq(width=w, height=h, spp=spp, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        ref, stats = o.render(req, threads=16)
        o.close()
        _REFS[key] = (ref.reshape(h, w, 4), stats)
    return _REFS[key]


def render_against_oracle(name, leaf_max, acc, capfd, flags=0, size=(W, H, SPP)):
    """Render scene `name` on the tree of `leaf_max`, compare with the oracle on that tree, and
    return the pass log's instance and leaf lines, the stats and the tree's leaf sizes."""
    w, h, spp = size
    host = host_of(name, leaf_max, w / h)
    sizes = leaf_sizes(host)
    stack = (host.stack_bound, centre_ray_stack_depth(host)) if name == "chain" else None
    r = GPURenderer(scene_of(name), w, h, spp, host_scene=host, tuning=N.tuning(flags=flags | N.TUNE_PASS_LOG), accumulation=acc)
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    ref, ostats = oracle_ref(name, leaf_max, acc, size)
    assert_parity(img, ref, r.stats, ostats)
    stats = dict(r.stats)
    r.close()
    trace, leaves, addr = log_line(err, "IZPI_TRACE_INSTANCE"), log_line(err, "IZPI_TRACE_LEAVES"), log_line(err, "IZPI_TRACE_ADDR")
    assert leaves["leaf_max"] == max(sizes), (leaves, sizes)
    assert leaves["leaf3"] == int(trace["dist"] == 1 and max(sizes) <= 3 and not flags & N.TUNE_LEAF4), (leaves, trace, sizes)
    return trace, leaves, stats, sizes, (addr, stack)


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("leaf_max,flags", [(1, 0), (2, 0), (2, N.TUNE_LEAF4), (3, 0), (4, 0)],
                         ids=["leaf1", "leaf2", "leaf2_form4", "leaf3", "leaf4"])
def test_grid_leaf_sizes_bitwise(gpu, capfd, acc, leaf_max, flags):
    """The 102-primitive grid (past the LDS limit: the ray-in-LDS instance C3 runs) on trees of at
    most 1, 2, 3 and 4 primitives per leaf: the form for three and, with 4, the general one, which
    must meet a leaf of exactly four; one tree on both forms (IZPI_TUNE_LEAF4)."""
    trace, leaves, stats, sizes, _ = render_against_oracle("grid", leaf_max, acc, capfd, flags)
    assert (trace["lds_bvh"], trace["ray_lds"], trace["tri"]) == (0, 1, 1), trace
    assert max(sizes) <= leaf_max and leaves["tmin_fixed"] == 1, (sizes, leaves)
    if leaf_max == 4:
        assert 4 in sizes and leaves["leaf3"] == 0, (sizes, leaves)
    else:
        assert leaves["leaf3"] == int(flags == 0), leaves
    assert stats["prim_steps"] > 0 and stats["leaf_shortcuts"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", [0, N.TUNE_NO_LDS_BVH], ids=["lds_tree", "global_tree"])
def test_root_leaf_bitwise(gpu, capfd, acc, flags):
    """One triangle: the root is a leaf of one primitive, entered by its own re-test, never by a
    shortcut."""
    trace, leaves, stats, sizes, _ = render_against_oracle("one", None, acc, capfd, flags)
    assert sizes == [1] and leaves["leaf3"] == 1 and trace["lds_bvh"] == int(flags == 0), (sizes, leaves, trace)
    assert stats["tri_tests"] > 0 and stats["leaf_shortcuts"] == 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("leaf_max,flags", [(3, 0), (3, N.TUNE_LEAF4), (4, 0)], ids=["leaf3", "leaf3_form4", "leaf4"])
def test_fan_full_batches_bitwise(gpu, capfd, acc, leaf_max, flags):
    """The fan: leaves of two and three (and, with 4, four) primitives, most lanes scanning at
    once. At this size a wave holds 16 rays, so a batch is at most full (16 x 4 = 64)."""
    trace, leaves, stats, sizes, _ = render_against_oracle("fan", leaf_max, acc, capfd, flags)
    assert max(sizes) == leaf_max and {2, 3} <= set(sizes), sizes
    assert (trace["lds_bvh"], trace["tri"]) == (0, 1), trace
    assert stats["prim_steps"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("leaf_max", [3, 4], ids=["leaf3", "leaf4"])
def test_fan_overfull_batches_bitwise(gpu, capfd, acc, leaf_max):
    """The fan at 320 x 256 x 2: waves of 32 and more rays whose scanning lanes hold more than 64
    pending tests, so a step serves the first lanes that fit and leaves the others scanning."""
    trace, leaves, stats, sizes, _ = render_against_oracle("fan", leaf_max, acc, capfd, size=BIG)
    assert max(sizes) == leaf_max and leaves["leaf3"] == int(leaf_max == 3), (sizes, leaves)
    assert stats["prim_steps"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", [0, N.TUNE_NO_RAY_LDS], ids=["ray_lds", "ray_global"])
def test_glass_pane_explicit_tmin_bitwise(gpu, capfd, acc, flags):
    """Triangles only, with a dielectric: path-length rays carry tMin 0, so the step takes each
    test's tMin from its owner's kind word and entry, with the ray in LDS and without; leaves of
    at most three (the form for three)."""
    trace, leaves, stats, sizes, _ = render_against_oracle("glass_pane", 3, acc, capfd, flags)
    assert (leaves["leaf3"], leaves["tmin_fixed"], trace["tri"]) == (1, 0, 1), (leaves, trace)
    assert (trace["lds_bvh"], trace["ray_lds"]) == (0, int(flags == 0)), trace  # 52 primitives: past the LDS limit
    assert stats["prim_steps"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("name,leaf_max,flags", [("spheres", 3, 0), ("spheres", 3, N.TUNE_NO_LDS_BVH), ("spheres", 4, N.TUNE_NO_LDS_BVH),
                                                 ("spheres_glass", 3, 0), ("spheres_glass", 3, N.TUNE_NO_LDS_BVH)],
                         ids=["lds_tree", "global_tree", "global_tree_leaf4", "glass_lds_tree", "glass_global_tree"])
def test_spheres_accept_loop_bitwise(gpu, capfd, acc, name, leaf_max, flags):
    """Spheres among the triangles: the owners' accept loop for both kinds (two roots per sphere,
    strict bounds), with the fixed tMin and, with a glass sphere, the explicit one."""
    trace, leaves, stats, sizes, _ = render_against_oracle(name, leaf_max, acc, capfd, flags)
    assert trace["tri"] == 0 and trace["lds_bvh"] == int(flags == 0), trace
    assert leaves["tmin_fixed"] == int(name == "spheres") and leaves["leaf3"] == int(max(sizes) <= 3), (leaves, sizes)
    assert stats["sph_tests"] > 0 and stats["tri_tests"] > 0


@pytest.mark.gpu
@ACCS
def test_nested_chain_spills_the_ring_bitwise(gpu, capfd, acc):
    """The nested chain on the reference builder's tree: a stack deeper than the ring, so the
    node step's lanes (taken from the mode mask) spill and the pops read back."""
    trace, leaves, stats, sizes, (addr, stack) = render_against_oracle("chain", None, acc, capfd)
    assert trace["lds_bvh"] == 0 and stack[0] > addr["ring"] and stack[1] > addr["ring"], (trace, addr, stack)
    assert stats["leaf_shortcuts"] > 0
