"""The staged form of the forward Colour k_shade (shade.h: stage_put, block_reserve_fwd,
stage_flush): every other block-iteration keeps its continuing entries in LDS and the next
one reserves output entries for both with one atomic.

Which entries a block gets does not change the image, so every case renders a small
forward Colour scene of triangles (more than 64 primitives: none staged in LDS; the last two
cases are a Spectral scene, which has no staged form, and the Cornell box alone, which gives
up its primitives' LDS copy for it) with the staged form and with IZPI_TUNE_NO_SHADE_STAGE
and asserts
* both canvases bitwise equal to each other and to the oracle's forward form,
* the counters rays, node_visits, tri_tests, light_tri_tests and launches equal,
* the pass log's IZPI_SHADE_FORM line naming the expected form.
"""
import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "node_visits", "tri_tests", "light_tri_tests")


def small_dragon(look_at=None):
    """The forward suite's dragon stand-in at 12 * 8 * 8 triangles in the RGB Cornell box;
    `look_at` turns the camera."""
    s = configs.cornell_dragon(1.0, n=8)
    if look_at is not None:
        s.set_camera((50, 50, -140), look_at, (0, 1, 0), 40, 1.0, 0, 10, 0, 1, 1.0)
    return s


def oracle_forward(scene, W, H, spp, max_depth):
    o = O.OracleScene(scene, aspect_override=W / H)
    req = N.RenderReq(width=W, height=H, spp=spp, max_depth=max_depth, sampler=N.SAMPLER_COLOUR, seed=12345,
                      abi_version=N.IZPI_ABI_VERSION, accumulation=N.ACC_FORWARD)
    canvas, st = o.render(req, threads=16)
    o.close()
    return canvas.reshape(H, W, 4), st


def form_lines(err):
    return [l for l in err.splitlines() if l.startswith("IZPI_SHADE_FORM")]


def bitwise_equal(a, b):
    x, y = a.view(np.uint64), b.view(np.uint64)
    bad = np.argwhere((x != y) & ~(np.isnan(a) & np.isnan(b)))
    assert len(bad) == 0, "not bit-identical: %d values differ, first %s" % (len(bad), bad[:5].tolist())


def render_both(scene, W, H, spp, max_depth, capfd, sampler=N.SAMPLER_COLOUR, **tune):
    """(canvas, stats, IZPI_SHADE_FORM lines) of the default form and of IZPI_TUNE_NO_SHADE_STAGE."""
    out = []
    r = GPURenderer(scene, W, H, spp, max_depth=max_depth, sampler=sampler, accumulation=N.ACC_FORWARD)
    for extra in (0, N.TUNE_NO_SHADE_STAGE):
        r.tuning = N.tuning(flags=N.TUNE_PASS_LOG | extra, **tune)
        capfd.readouterr()
        img = r.render()
        out.append((img, r.stats, form_lines(capfd.readouterr().err)))
    r.close()
    return out


def check_case(scene, W, H, spp, capfd, max_depth=50, **tune):
    (a, sa, la), (b, sb, lb) = render_both(scene, W, H, spp, max_depth, capfd, **tune)
    assert la == ["IZPI_SHADE_FORM staged"], la
    assert lb == ["IZPI_SHADE_FORM plain (IZPI_TUNE_NO_SHADE_STAGE)"], lb
    ref, rs = oracle_forward(scene, W, H, spp, max_depth)
    bitwise_equal(a, b)
    bitwise_equal(a, ref)
    for k in COUNTERS:
        assert sa[k] == sb[k] == rs[k], (k, sa[k], sb[k], rs[k])
    assert sa["launches"] == sb["launches"], (sa["launches"], sb["launches"])
    return sa


def test_stage_one_partial_iteration(gpu, capfd):
    """128 units: one block, one partial iteration, staged and flushed after the loop."""
    check_case(small_dragon(), 8, 8, 2, capfd)


def test_stage_odd_and_even_trip_counts(gpu, capfd):
    """524,288 units against a resident grid of 768 blocks x 256 lanes: the first passes'
    blocks run 3 iterations (stage, reserve, stage + the flush after the loop) or 2."""
    check_case(small_dragon(), 512, 512, 2, capfd)


@pytest.mark.parametrize("slots,W,spp", [(300, 48, 4), (65536, 256, 4)])
def test_stage_few_slots(gpu, capfd, slots, W, spp):
    """Far fewer slots than units: many passes whose k_refill appends camera entries behind
    the staged form's output, then the drain once the units run out."""
    st = check_case(small_dragon(), W, W, spp, capfd, slots=slots)
    assert st["slots"] == max(slots, 1024)  # (the library's smallest queue)
    assert st["launches"] > W * W * spp // st["slots"]  # (every unit went through the queue)


@pytest.mark.parametrize("max_depth", [0, 1])
def test_stage_every_path_ends(gpu, capfd, max_depth):
    """maxDepth 0 and 1: no path continues, so nothing is staged or reserved (no atomic)
    and every pass leaves an empty queue to k_refill."""
    check_case(small_dragon(), 32, 32, 4, capfd, max_depth=max_depth, slots=300)


def test_stage_geometry_in_part_of_the_frame(gpu, capfd):
    """The camera turned away so that half the frame misses the box: those paths end at
    once, so some iterations stage nothing and reserve something, others the reverse
    (294,912 units: 384 of the 768 blocks run two iterations in the first pass)."""
    check_case(small_dragon(look_at=(130, 50, 0)), 384, 384, 2, capfd)


def test_stage_ineligible_scene_keeps_plain_form(gpu, capfd):
    """The Spectral sampler has no staged instance (its entries carry cold records and its
    arena the Spectral tables): both settings run the plain form, and say so."""
    (a, sa, la), (b, sb, lb) = render_both(configs.cornell_glass_spectral(), 32, 32, 4, 50, capfd, sampler=N.SAMPLER_SPECTRAL)
    assert la == lb == ["IZPI_SHADE_FORM plain (no staged instance)"], (la, lb)
    bitwise_equal(a, b)


def test_stage_small_lambert_scene_gives_up_primitive_staging(gpu, capfd):
    """The Cornell box alone (at most 64 primitives, Lambert and light only) would stage its
    primitives' records where the output stage lies; it runs the staged form without them,
    and with IZPI_TUNE_NO_SHADE_STAGE the plain form with them, both as the oracle."""
    check_case(configs.cornell_rgb(), 64, 64, 4, capfd)
