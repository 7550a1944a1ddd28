"""One render per shading instance the instance rule can return (wavefront.hip: shade_instance),
13 in all: Colour recursive x {CONST, BASIC, SURF, FULL}, Colour forward x {BASIC, SURF, FULL},
Spectral x {BASIC, SURF, FULL} x {recursive, forward}; and k_tail's deep-stack instance
(`tail=64`) once per accumulation.

Every render runs under IZPI_TUNE_PASS_LOG and must
* name the expected instance in its IZPI_SHADE_INSTANCE line (the forward Colour BASIC and SURF
  renders also their staged form, IZPI_SHADE_FORM staged), so that a scene that slips to
  another instance fails here instead of passing on the other kernels;
* equal the CPU oracle in the same accumulation: the image bit for bit and the counters
  (assert_parity).

The SURF scene of the Colour sampler is cornell_pbr's box without its spheres and with a small
metal mesh: the staged form takes a scene of triangles alone (no ray times in the entries) with
more than 64 primitives (none staged in LDS behind the Colour tables).

The deep-stack scene is deep_line_scene's geometry (test_gpu_trace_steps.py) under a comb-shaped
tree: the reference builder's median splits keep the stack bound at 19 for 20,000 triangles and
at 24 for 200,000, so the bound past 32 comes from the tree: every inner node holds the next
inner node in slot 0 and three leaves, and a ray along the camera's axis, which hits every box,
pushes three entries per level on its first descent.
"""
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer
from izpi_amd.scene import HostScene, Scene
from oracle import oracle as O
from tests import table_cases as T
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_parity_materials import rgb_glass_box, spectral_pbr_box, textured_lambert_box
from tests.test_gpu_trace_steps import deep_line_scene

W, H, SPP, MAX_DEPTH, SEED = 32, 32, 4, 50, 12345
ACCS = {"rec": N.ACC_RECURSIVE, "fwd": N.ACC_FORWARD}
SAMPLERS = {"colour": N.SAMPLER_COLOUR, "spectral": N.SAMPLER_SPECTRAL}


def pbr_triangle_box():
    s = configs.cornell_pbr(1.0, res=16)
    metal = int(s.spheres["material"][-1])
    s.spheres = s.spheres[:0]
    s.add_triangles(*configs.dragon_mesh(3), metal)
    return s


def spectral_lambert_box():
    s = Scene("spectral_lambert")
    configs.add_box(s, T.spectral_box_materials(s))
    configs.cornell_camera(s, 1.0)
    return s


# instance -> the scene that runs it
SCENES = {
    "colour/rec/CONST": configs.cornell_rgb,
    "colour/rec/BASIC": textured_lambert_box,
    "colour/rec/SURF": pbr_triangle_box,
    "colour/rec/FULL": lambda: rgb_glass_box(True),
    "colour/fwd/BASIC": configs.cornell_rgb,
    "colour/fwd/SURF": pbr_triangle_box,
    "colour/fwd/FULL": lambda: rgb_glass_box(True),
    "spectral/rec/BASIC": spectral_lambert_box,
    "spectral/rec/SURF": lambda: spectral_pbr_box(True),
    "spectral/rec/FULL": configs.cornell_glass_spectral,
    "spectral/fwd/BASIC": spectral_lambert_box,
    "spectral/fwd/SURF": lambda: spectral_pbr_box(True),
    "spectral/fwd/FULL": configs.cornell_glass_spectral,
}
STAGED = ("colour/fwd/BASIC", "colour/fwd/SURF")


def render_logged(scene, w, h, spp, sampler, acc, capfd, host_scene=None):
    """(canvas, stats, pass log) of one frame under IZPI_TUNE_PASS_LOG."""
    r = GPURenderer(scene, w, h, spp, max_depth=MAX_DEPTH, sampler=sampler, seed=SEED, accumulation=acc,
                    tuning=N.tuning(flags=N.TUNE_PASS_LOG), host_scene=host_scene)
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    stats = r.stats
    r.close()
    return img, stats, err


def oracle_frame(scene, w, h, spp, sampler, acc, tree=None):
    o = O.OracleScene(scene, aspect_override=w / h)
    if tree is not None:
        o.set_bvh(*tree)
    req = N.RenderReq(width=w, height=h, spp=spp, max_depth=MAX_DEPTH, sampler=sampler, seed=SEED,
                      abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
    ref, stats = o.render(req, threads=16)
    o.close()
    return ref.reshape(h, w, 4), stats


def lines(err, key):
    return [l for l in err.splitlines() if l.startswith(key + " ")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_shade_instance_bitwise(gpu, capfd, name):
    sampler, acc = SAMPLERS[name.split("/")[0]], ACCS[name.split("/")[1]]
    scene = SCENES[name]()
    img, stats, err = render_logged(scene, W, H, SPP, sampler, acc, capfd)
    assert lines(err, "IZPI_SHADE_INSTANCE") == ["IZPI_SHADE_INSTANCE %s tail=32" % name], err
    if name in STAGED:
        assert lines(err, "IZPI_SHADE_FORM") == ["IZPI_SHADE_FORM staged"], err
    ref, ostats = oracle_frame(scene, W, H, SPP, sampler, acc)
    assert_parity(img, ref, stats, ostats)


def comb_tree(boxes, leaf=3):
    """A BVH4 over `boxes` ([n][6] f64, primitive order kept) as a comb: inner node i at index
    4 i holds inner node i + 1 in slot 0 and three leaves of `leaf` primitives in slots 1..3;
    the last one holds the remaining leaves (at most 4). (nodes, order) as izpi_host_scene_set_bvh
    takes them; the stack bound is 3 per inner node."""
    node_t = np.dtype([("mn", "<f4", (3, 4)), ("mx", "<f4", (3, 4)), ("child", "<i4", 4), ("pc", "<i4", 4)])
    n = len(boxes)
    lo = np.nextafter(boxes[:, :3].astype(np.float32), np.float32(-np.inf))  # f32 boxes that hold the f64 ones
    hi = np.nextafter(boxes[:, 3:].astype(np.float32), np.float32(np.inf))
    ranges = [(a, min(a + leaf, n)) for a in range(0, n, leaf)]
    inner = max(1, -(-(len(ranges) - 4) // 3) + 1)
    nodes = np.zeros(4 * (inner - 1) + 1 + len(ranges) - 3 * (inner - 1), node_t)
    nodes["child"] = -1
    rest_lo, rest_hi = lo.min(0), hi.max(0)  # (every inner slot-0 box: the whole scene, a superset of its subtree)

    def put_leaf(at, parent, slot, rng):
        a, b = rng
        bl, bh = lo[a:b].min(0), hi[a:b].max(0)
        nodes[at]["mn"][:, 0], nodes[at]["mx"][:, 0] = bl, bh
        nodes[at]["child"][0], nodes[at]["pc"][0] = a, b - a
        nodes[parent]["mn"][:, slot], nodes[parent]["mx"][:, slot] = bl, bh
        nodes[parent]["child"][slot] = at

    for i in range(inner):
        at = 4 * i
        if i + 1 < inner:
            nodes[at]["mn"][:, 0], nodes[at]["mx"][:, 0] = rest_lo, rest_hi
            nodes[at]["child"][0] = at + 4
            for k in range(3):
                put_leaf(at + 1 + k, at, 1 + k, ranges[3 * i + k])
        else:
            for k, rng in enumerate(ranges[3 * i:]):
                put_leaf(at + 1 + k, at, k, rng)
    return nodes.view(np.uint8).reshape(-1, 128), np.arange(n, dtype=np.uint32)


_DEEP = {}


def deep_scene():
    """(scene, tree) of the deep-stack cases, built once."""
    if not _DEEP:
        scene = deep_line_scene(100)
        host = HostScene(scene, aspect_override=1.0)
        _DEEP["scene"], _DEEP["tree"] = scene, comb_tree(host.prim_boxes())
    return _DEEP["scene"], _DEEP["tree"]


def test_deep_scene_stack_bound():
    scene, tree = deep_scene()
    host = HostScene(scene, aspect_override=1.0)
    host.set_bvh(*tree)
    assert 32 < host.stack_bound <= 64, host.stack_bound


@pytest.mark.gpu
@pytest.mark.parametrize("acc", ["rec", "fwd"])
def test_deep_stack_tail_instance_bitwise(gpu, capfd, acc):
    scene, tree = deep_scene()
    host = HostScene(scene, aspect_override=1.0)
    host.set_bvh(*tree)
    assert host.stack_bound > 32
    img, stats, err = render_logged(scene, 16, 16, 2, N.SAMPLER_COLOUR, ACCS[acc], capfd, host_scene=host)
    want = "colour/rec/CONST" if acc == "rec" else "colour/fwd/BASIC"
    assert lines(err, "IZPI_SHADE_INSTANCE") == ["IZPI_SHADE_INSTANCE %s tail=64" % want], err
    assert stats["tail_ms"] > 0, stats
    ref, ostats = oracle_frame(scene, 16, 16, 2, N.SAMPLER_COLOUR, ACCS[acc], tree=tree)
    assert_parity(img, ref, stats, ostats)


def test_forward_renders_launch_no_k_start():
    """The recorded kernel traces of profiles/r11a/ (one small frame per render, this commit):
    the forward renders' kernel names hold no k_start, the recursive ones' do."""
    d = Path(__file__).resolve().parents[1] / "profiles" / "r11a"
    names = {p.stem[len("launches_new_"):]: {l.split()[0] for l in p.read_text().splitlines() if l.strip()}
             for p in sorted(d.glob("launches_new_*.txt"))}
    assert sorted(names) == ["colour_fwd", "colour_rec", "spectral_fwd", "spectral_rec"], sorted(names)
    for render, ks in names.items():
        started = any(k.startswith("k_start") for k in ks)
        assert started == render.endswith("_rec"), (render, sorted(ks))
        assert any(k.startswith("k_shade") for k in ks) and any(k.startswith("k_accumulate") for k in ks), (render, sorted(ks))
