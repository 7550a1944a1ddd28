"""k_trace2's record addressing: 32-bit byte offsets from a scalar base where the uploaded
scene's node block and primitive records each stay under 4 GiB (DevScene::addr32), 64-bit
addresses otherwise (IZPI_TUNE_WIDE_ADDR forces them on a small scene).

Each render is 40 x 30 pixels at 2 spp, in both accumulation modes, against the CPU oracle on
the same tree: image bit for bit and counters equal (assert_parity). The scenes are the ones an
offset can go wrong on: a root that is a leaf (no inner node: leaf lanes read the dummy one), a
tree past the 4-KB LDS limit without and with (u, v) (the ray-in-LDS instance C3 runs, and the
one that re-reads rays from global memory), and a stack deeper than the instance's ring (spill and
read-back). The 4-GiB predicate is checked on the host with fabricated sizes.
"""
import subprocess
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
from tests.test_gpu_trace_steps import centre_ray_stack_depth

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP = 40, 30, 2
ACCS = pytest.mark.parametrize("acc", [N.ACC_FORWARD, N.ACC_RECURSIVE], ids=["forward", "recursive"])

_SCENES = {}
_REFS = {}


def one_triangle_scene():
    """One emitting triangle in front of the camera: the tree's root is a leaf."""
    s = configs.Scene("one_triangle")
    light = s.diffuse_light(emit=s.constant((2.0, 1.5, 1.0)))
    s.add_triangles([(10, 10, 50)], [(90, 15, 55)], [(45, 90, 60)], light)
    configs.cornell_camera(s, W / H)
    return s


def grid_scene(textured):
    """A tilted, uneven 10 x 5 grid of quads (100 triangles) under a two-triangle light: 102
    primitives, 11 KB of leaf and primitive records, past the 4 KB an LDS-resident tree may have.
    textured: the grid's albedo is an image, so hits carry (u, v)."""
    s = configs.Scene("grid_uv" if textured else "grid")
    light = s.diffuse_light(emit=s.constant((15.0, 15.0, 15.0)))
    if textured:
        y, x = np.mgrid[0:16, 0:16] / 16.0
        img = np.stack([0.2 + 0.6 * x, 0.3 + 0.5 * y, 0.25 + 0.5 * ((np.floor(8 * x) + np.floor(8 * y)) % 2), np.ones_like(x)], -1)
        mat = s.lambert(albedo=s.image(img))
    else:
        mat = s.lambert(albedo=s.constant((0.7, 0.6, 0.5)))
    def p(i, j):
        return (5.0 + 9.0 * i + 0.7 * ((3 * i + 5 * j) % 4), 8.0 + 16.0 * j + 0.9 * ((i + 2 * j) % 3), 40.0 + 2.5 * i + 1.5 * j)
    v0, v1, v2, uv = [], [], [], []
    for i in range(10):
        for j in range(5):
            a, b, c, d = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            ua, ub, uc, ud = (i / 10, j / 5), ((i + 1) / 10, j / 5), ((i + 1) / 10, (j + 1) / 5), (i / 10, (j + 1) / 5)
            v0 += [a, a]; v1 += [b, c]; v2 += [c, d]
            uv += [[*ua, *ub, *uc], [*ua, *uc, *ud]]
    s.add_triangles(v0, v1, v2, mat, uv=uv if textured else None)
    s.add_triangles([(20, 99, 20), (20, 99, 20)], [(80, 99, 20), (80, 99, 35)], [(80, 99, 35), (20, 99, 35)], light)
    configs.cornell_camera(s, W / H)
    return s


def nested_chain_scene(n=20000):
    """n thin triangles nested along the camera's axis, each a little smaller than the one before:
    the ray along the axis hits every box on its first descent and holds more stack entries than
    the ring has."""
    s = configs.Scene("nested_chain")
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    k = np.arange(n) / n
    z = 10.0 + 80.0 * k
    r = 30.0 - 12.0 * k
    v0 = np.stack([50.0 - r, 50.0 - r, z], -1)
    v1 = np.stack([50.0 + r, 50.0 - r, z], -1)
    v2 = np.stack([np.full(n, 50.0), 50.0 + r, z + 0.001], -1)
    s.add_triangles(configs.f32(v0), configs.f32(v1), configs.f32(v2), mats["White"])
    configs.cornell_camera(s, W / H)
    return s


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = {"one": one_triangle_scene, "grid": lambda: grid_scene(False), "grid_uv": lambda: grid_scene(True),
                         "chain": nested_chain_scene}[name]()
    return _SCENES[name]


def oracle_ref(name, acc):
    """The oracle's canvas and counters of scene `name`, computed once per accumulation mode."""
    if (name, acc) not in _REFS:
        o = O.OracleScene(scene_of(name), aspect_override=W / H)
        req = N.RenderReq(width=W, height=H, spp=SPP, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        ref, stats = o.render(req, threads=16)
        o.close()
        _REFS[(name, acc)] = (ref.reshape(H, W, 4), stats)
    return _REFS[(name, acc)]


def render_against_oracle(name, acc, capfd, flags=0):
    """Render `name`, compare with the oracle, and return the pass log's instance and addressing."""
    r = GPURenderer(scene_of(name), W, H, SPP, tuning=N.tuning(flags=flags | N.TUNE_PASS_LOG), accumulation=acc)
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    ref, ostats = oracle_ref(name, acc)
    assert_parity(img, ref, r.stats, ostats)
    stats = dict(r.stats)
    r.close()
    return log_line(err, "IZPI_TRACE_INSTANCE"), log_line(err, "IZPI_TRACE_ADDR"), stats


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", [0, N.TUNE_NO_LDS_BVH, N.TUNE_NO_LDS_BVH | N.TUNE_WIDE_ADDR], ids=["lds_tree", "global_tree", "global_tree_wide"])
def test_root_leaf_bitwise(gpu, capfd, acc, flags):
    """One triangle: the root is a leaf, the scene has no inner node. From global memory the leaf
    lanes' unused loads go to the dummy inner record at offset 0 of the node block."""
    host = HostScene(scene_of("one"), aspect_override=W / H)
    nodes = np.frombuffer(host.nodes().tobytes(), dtype=np.dtype([("b", "<f4", (6, 4)), ("child", "<i4", 4), ("pc", "<i4", 4)]))
    assert len(nodes) == 1 and nodes[0]["pc"][0] == 1
    trace, addr, stats = render_against_oracle("one", acc, capfd, flags)
    assert trace["lds_bvh"] == int(flags == 0) and addr["a32"] == int(flags == N.TUNE_NO_LDS_BVH), (trace, addr)
    assert stats["tri_tests"] > 0


@pytest.mark.gpu
@ACCS
@pytest.mark.parametrize("flags", [0, N.TUNE_WIDE_ADDR], ids=["offsets32", "wide"])
def test_grid_ray_in_lds_bitwise(gpu, capfd, acc, flags):
    """About 100 triangles without (u, v): the global-memory instance with the rays in LDS, which
    C3 runs, on 32-bit offsets and on the 64-bit addresses of a scene past 4 GiB."""
    trace, addr, stats = render_against_oracle("grid", acc, capfd, flags)
    assert (trace["lds_bvh"], trace["ray_lds"], trace["tri"]) == (0, 1, 1), trace
    assert addr["a32"] == int(flags == 0), addr
    assert stats["node_steps"] > 0 and stats["prim_steps"] > 0


WIDE = pytest.mark.parametrize("wide", [0, N.TUNE_WIDE_ADDR], ids=["offsets32", "wide"])


@pytest.mark.gpu
@ACCS
@WIDE
def test_grid_textured_bitwise(gpu, capfd, acc, wide):
    """The same grid under an image texture: hits carry (u, v), the rays stay in global memory."""
    trace, addr, stats = render_against_oracle("grid_uv", acc, capfd, wide)
    assert (trace["lds_bvh"], trace["ray_lds"], addr["a32"]) == (0, 0, int(wide == 0)), (trace, addr)
    assert stats["prim_steps"] > 0


@pytest.mark.gpu
@ACCS
@WIDE
def test_nested_chain_spills_the_ring_bitwise(gpu, capfd, acc, wide):
    """A stack deeper than the instance's ring (the pass log gives its size): the oldest entries
    go to the spill area and come back."""
    host = HostScene(scene_of("chain"), aspect_override=W / H)
    trace, addr, _ = render_against_oracle("chain", acc, capfd, wide)
    assert (trace["lds_bvh"], addr["a32"]) == (0, int(wide == 0)), (trace, addr)
    assert host.stack_bound > addr["ring"] and centre_ray_stack_depth(host) > addr["ring"], (host.stack_bound, addr)


def test_addr32_predicate_limits(tmp_path):
    """trace_addr32 at the limit: a node block or primitive array of at most 4 GiB qualifies, one
    record more does not; the block's layout is inner nodes, quantised nodes, leaf records."""
    exe = tmp_path / "trace_addr32_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "trace_addr32_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {}
    for line in out.splitlines():
        name, *f = line.replace("->", "").split()
        inner, innerq, leaves, prims, innerq_at, leaves_at, nbytes, ok = map(int, f)
        assert (innerq_at, leaves_at, nbytes) == (128 * inner, 128 * inner + 64 * innerq, 128 * inner + 64 * innerq + 32 * leaves), line
        assert ok == int(nbytes <= 2 ** 32 and 80 * prims <= 2 ** 32), line
        got[name] = ok
    assert got == {"empty": 1, "c3_like": 1, "inner_at_limit": 1, "inner_over": 0, "leaves_at_limit": 1, "leaves_over": 0,
                   "quantised_at_limit": 1, "quantised_over": 0, "prims_under": 1, "prims_over": 0, "far_over": 0}, got
