"""One context through every way a render call is driven (one shot, a preview sampler, a
progressive session's begin and steps): the Colour frames between them keep their workspace
plan, allocate nothing and repeat the first frame bit for bit."""
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 30, 4


def test_colour_preview_session_colour_on_one_context(gpu):
    r = GPURenderer(configs.cornell_rgb(), W, H, SPP, accumulation=N.ACC_FORWARD, tuning=N.tuning(slots=2000))
    first = r.render()
    plan = (r.stats["slots"], r.stats["chunk_spp"])
    assert plan == (2000, SPP)

    def colour_again():
        img = r.render()
        assert (r.stats["slots"], r.stats["chunk_spp"]) == plan
        assert r.stats["alloc_ms"] < 0.5, r.stats["alloc_ms"]
        assert img.tobytes() == first.tobytes()

    r.sampler = N.SAMPLER_WIREFRAME
    wire = r.render()
    assert r.stats["rays"] == r.stats["samples"] == W * H * SPP and wire.tobytes() != first.tobytes()
    r.sampler = N.SAMPLER_COLOUR
    colour_again()
    with r.progressive(2) as s:  # begin, two steps of 2 spp, end
        s.step()
        assert s.step() == SPP
        assert s.stats["slots"] == plan[0]
        assert s.snapshot().tobytes() == first.tobytes()
    colour_again()
    r.close()


def test_use_tree_loads_what_a_fresh_renderer_loads(gpu):
    """use_tree goes through the constructor's scene loader: after each of its three branches
    (the GPU-built tree, the quantised upload, back to the reference tree) the context renders
    the frame, counts the work and names the tree like a renderer opened with those arguments."""
    scene = configs.cornell_dragon(1.0, n=24)
    r = GPURenderer(scene, 32, 32, 2, bvh="reference")
    r.render()
    for tree in (dict(bvh="gpu"), dict(bvh="gpu", bvh_quantized=True), dict(bvh="reference")):
        r.use_tree(scene, **tree)
        img = r.render()
        fresh = GPURenderer(scene, 32, 32, 2, **tree)
        assert img.tobytes() == fresh.render().tobytes(), tree
        for k in ("rays", "node_visits", "tri_tests", "light_tri_tests"):
            assert r.stats[k] == fresh.stats[k], (tree, k)
        assert (r.bvh_leaf_max, r.bvh_quantized) == (fresh.bvh_leaf_max, fresh.bvh_quantized), tree
        assert (r.bvh_build_ms is None) == (fresh.bvh_build_ms is None) == (tree["bvh"] == "reference"), tree
        fresh.close()
    r.close()
