"""k_trace2's node step, primitive step and refill on the paths a change of their instruction
sequences can break: leaf sizes 1..4 with primitive batches over 64 tests (lanes not served),
the scheduling knobs at both ends, a tree deeper than the 16-entry stack ring (spill and
read-back), a queue shorter than one chunk, an axis-exact camera, lanes on the scalar-twin slab
beside lanes on the packed one, and the BVH-in-LDS instances with the rays in LDS and without.

Every case is a render against the CPU oracle on the same tree: image bit for bit, and the
counters (rays, node visits, triangle and sphere tests) equal, as assert_parity checks. The
renders run the instances a frame runs (izpi_gpu_trace asks for (u, v) and so never runs the
ray-in-LDS instance); one izpi_gpu_trace case adds waves that mix the two slab forms.
"""
import ctypes as C

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer
from izpi_amd.scene import HostScene
from oracle import oracle as O
from tests.table_cases import log_line
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

_SCENES = {}
_REFS = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = {"dragon": lambda: configs.cornell_dragon(1.0, n=60), "deep": deep_line_scene,
                         "axis": axis_camera_scene, "cornell": configs.cornell_rgb,
                         "pbr": lambda: configs.cornell_pbr(1.0, res=64)}[name]()
    return _SCENES[name]


def oracle_ref(name, W, H, spp, acc=N.ACC_RECURSIVE, tree=None, tree_key=None):
    """The oracle's canvas and counters of scene `name` (on `tree` = (nodes, order) when given),
    computed once per (scene, frame, accumulation, tree)."""
    key = (name, W, H, spp, acc, tree_key)
    if key not in _REFS:
        o = O.OracleScene(scene_of(name), aspect_override=W / H)
        if tree is not None:
            o.set_bvh(*tree)
        req = N.RenderReq(width=W, height=H, spp=spp, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        ref, stats = o.render(req, threads=16)
        o.close()
        _REFS[key] = (ref.reshape(H, W, 4), stats)
    return _REFS[key]


def deep_line_scene(n=20000):
    """The Cornell box with n thin triangles stacked along the camera's axis: a ray along it
    hits every box of the reference tree, whose first descent then holds 18 stack entries."""
    s = configs.Scene("deep_line")
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    z = 10.0 + 80.0 * np.arange(n) / n
    v0 = np.stack([np.full(n, 20.0), np.full(n, 20.0), z], -1)
    v1 = np.stack([np.full(n, 80.0), np.full(n, 20.0), z], -1)
    v2 = np.stack([np.full(n, 50.0), np.full(n, 80.0), z + 0.001], -1)
    s.add_triangles(configs.f32(v0), configs.f32(v1), configs.f32(v2), mats["White"])
    configs.cornell_camera(s, 1.0)
    return s


def axis_camera_scene():
    """The dragon box seen from inside, the camera looking exactly along +x."""
    s = configs.cornell_dragon(1.0, n=60)
    s.set_camera((5, 50, 50), (95, 50, 50), (0, 1, 0), 40, 1.0, 0, 10, 0, 1, 1.0)
    return s


def centre_ray_stack_depth(host):
    """Most stack entries BVH4.Hit holds for the ray from (50, 50, -140) along +z before any hit
    shortens it (bvh4.go:76-160: first hit child next, the others pushed in slot order)."""
    nd = np.frombuffer(host.nodes().tobytes(), dtype=np.dtype([("mn", "<f4", (3, 4)), ("mx", "<f4", (3, 4)),
                                                               ("child", "<i4", 4), ("pc", "<i4", 4)]))
    stack, cur, deepest = [], 0, 0
    while True:
        n = nd[cur]
        nxt = None
        if n["pc"][0] == 0:
            hs = [i for i in range(4) if n["child"][i] != -1 and n["mn"][0][i] <= 50 <= n["mx"][0][i]
                  and n["mn"][1][i] <= 50 <= n["mx"][1][i]]
            if hs:
                nxt = n["child"][hs[0]]
                stack.extend(n["child"][i] for i in hs[1:])
                deepest = max(deepest, len(stack))
        if nxt is None:
            if not stack:
                return deepest
            nxt = stack.pop()
        cur = nxt


@pytest.mark.parametrize("leaf_max", [1, 2, 3, 4, "reference"])
def test_leaf_sizes_bitwise(gpu, leaf_max):
    """Leaves of at most 1, 2, 3 and 4 primitives on the GPU-built tree, and the reference tree:
    the distributed primitive step ranks 1..4 tests per lane, and a wave whose lanes ask for
    more than 64 leaves the last ones unserved for a step."""
    W, H, spp = 64, 64, 4
    if leaf_max == "reference":
        r = GPURenderer(scene_of("dragon"), W, H, spp)
        ref, ostats = oracle_ref("dragon", W, H, spp)
    else:
        r = GPURenderer(scene_of("dragon"), W, H, spp, bvh="gpu", bvh_leaf_max=leaf_max)
        ref, ostats = oracle_ref("dragon", W, H, spp, tree=(r.bvh_nodes(), r.host._bvh_keep[1]), tree_key=leaf_max)
    img = r.render()
    assert_parity(img, ref, r.stats, ostats)
    assert r.stats["prim_steps"] > 0 and r.stats["node_steps"] > 0
    r.close()


@pytest.mark.parametrize("acc", [N.ACC_FORWARD, N.ACC_RECURSIVE], ids=["forward", "recursive"])
@pytest.mark.parametrize("tune", [{"refill_min": 1}, {"refill_min": 64}, {"trace_chunk": 1}, {"trace_chunk": 16},
                                  {"prim_weight": 1}, {"prim_weight": 100000}],
                         ids=lambda t: "%s=%d" % next(iter(t.items())))
def test_step_scheduling_knobs_bitwise(gpu, tune, acc):
    """When a wave refills, how much it dequeues and which step it picks are scheduling only:
    image and counters stay the oracle's at both ends of each knob, in both accumulations."""
    W, H, spp = 64, 64, 4
    r = GPURenderer(scene_of("dragon"), W, H, spp, tuning=N.tuning(**tune), accumulation=acc)
    img = r.render()
    ref, ostats = oracle_ref("dragon", W, H, spp, acc)
    assert_parity(img, ref, r.stats, ostats)
    r.close()


def test_tree_deeper_than_the_ring_bitwise(gpu):
    """A traversal that holds more than 16 stack entries spills the ring's oldest ones to global
    memory and reads them back on pop."""
    W, H, spp = 16, 16, 2
    host = HostScene(scene_of("deep"), aspect_override=1.0)
    assert host.stack_bound > 16 and centre_ray_stack_depth(host) > 16
    r = GPURenderer(scene_of("deep"), W, H, spp)
    img = r.render()
    ref, ostats = oracle_ref("deep", W, H, spp)
    assert_parity(img, ref, r.stats, ostats)
    r.close()


def test_queue_shorter_than_a_chunk_bitwise(gpu):
    """64 camera rays: fewer than one chunk, most waves find no work, one refills partly."""
    r = GPURenderer(scene_of("dragon"), 8, 8, 1)
    img = r.render()
    ref, ostats = oracle_ref("dragon", 8, 8, 1)
    assert_parity(img, ref, r.stats, ostats)
    r.close()


def test_axis_exact_camera_bitwise(gpu):
    """A camera looking exactly along +x: its basis vectors hold exact zeros."""
    r = GPURenderer(scene_of("axis"), 16, 16, 2)
    img = r.render()
    ref, ostats = oracle_ref("axis", 16, 16, 2)
    assert_parity(img, ref, r.stats, ostats)
    r.close()


def test_slab_forms_mixed_in_one_wave_bitwise(gpu):
    """Every third ray has zero direction components (infinite f32 inverses: the scalar-twin
    slab), the others are ordinary, so each wave's node steps hold lanes of both kinds."""
    scene = scene_of("dragon")
    o = O.OracleScene(scene, aspect_override=1.0)
    r = GPURenderer(scene, 8, 8, 1)
    rng = np.random.default_rng(11)
    rays = []
    for i in range(3072):
        org = rng.uniform(5, 95, 3)
        if i % 3 == 0:
            d = np.zeros(3)
            d[(i // 3) % 3] = 1.0 if (i // 9) % 2 else -1.0
        else:
            d = rng.uniform(-1, 1, 3)
        rays.append(list(org) + list(d) + [0.001, 1e300])
    rays = np.ascontiguousarray(rays, np.float64)
    got = (N.Hit * len(rays))()
    assert N.lib().izpi_gpu_trace(r.ctx, rays.ctypes.data_as(C.POINTER(C.c_double)), len(rays), got) == 0
    want = o.trace(rays)
    nhit = 0
    for i in range(len(rays)):
        g, w = got[i], want[i]
        assert g.hit == w.hit, i
        if w.hit:
            nhit += 1
            assert g.prim_ref == w.prim_ref, i
            assert bytes(g)[:72] == bytes(w)[:72], i
    assert nhit > 2000
    r.close()
    o.close()


@pytest.mark.parametrize("flags", [0, N.TUNE_NO_RAY_LDS], ids=["ray_lds", "no_ray_lds"])
@pytest.mark.parametrize("which", ["cornell", "pbr"])
def test_lds_tree_instances_bitwise(gpu, capfd, which, flags):
    """The instances that traverse the tree from LDS, with the rays in LDS and without: the
    pass log names the instance that ran."""
    W, H, spp = 48, 48, 4
    r = GPURenderer(scene_of(which), W, H, spp, tuning=N.tuning(flags=flags | N.TUNE_PASS_LOG))
    capfd.readouterr()
    img = r.render()
    trace = log_line(capfd.readouterr().err, "IZPI_TRACE_INSTANCE")
    ref, ostats = oracle_ref(which, W, H, spp)
    assert_parity(img, ref, r.stats, ostats)
    r.close()
    assert (trace["lds_bvh"], trace["ray_lds"]) == (1, int(flags == 0)), trace
