"""Progressive rendering on the GPU (izpi_gpu_progressive_*, GPURenderer.progressive): a
session that has rendered k samples per pixel, in any split of steps, snapshots exactly the
canvas a one-shot render writes at spp = k, bit for bit and with the same counters.

The reference is the CPU oracle rendered at spp = done (never another GPU render), on the
scenes of tests/test_forward_accumulation.scene_case: 32x32, 40x40 or 30x20 at 8 spp.
"""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import GPURenderer, MultiGPURenderer, make_request
from oracle import oracle as O
from tests import preview_ref as PR
from tests.test_forward_accumulation import CASES, scene_case
from tests.test_gpu_forward import assert_bitwise, oracle_both

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ACCS = [N.ACC_RECURSIVE, N.ACC_FORWARD]


@functools.lru_cache(maxsize=None)
def scene_of(which):
    return scene_case(which)


@functools.lru_cache(maxsize=None)
def oracle_at(which, spp, tiles=None):
    """The oracle's ((recursive canvas, stats), (forward canvas, stats)) of a case at `spp`
    samples, computed once per session and shared (read only)."""
    scene, W, H, _, sampler = scene_of(which)
    t = None if tiles is None else np.array(tiles, np.uint32).reshape(-1, 4)
    return oracle_both(scene, W, H, spp, sampler, tiles=t)


def renderer(which, acc, **kw):
    scene, W, H, spp, sampler = scene_of(which)
    return GPURenderer(scene, W, H, spp, sampler=sampler, accumulation=acc, **kw)


def run_schedule(r, which, acc, step_spp, steps, **kw):
    """Steps of a session, a CANVAS snapshot after each against the oracle at spp = done."""
    with r.progressive(step_spp, **kw) as s:
        assert (s.done, s.total) == (0, 8)
        for n in steps:
            before = s.done
            assert s.step(n) == min(8, before + (n or step_spp))
            ref, ref_stats = oracle_at(which, s.done)[acc]
            assert_bitwise(s.snapshot(), ref, s.stats, ref_stats)
        return s.done


# ---- 1. any split equals one shot
@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("which", CASES)
def test_any_split_equals_one_shot(gpu, which, acc):
    """N = 8 in steps of step_spp = 3: 3, 3 and a last step clipped to 2."""
    r = renderer(which, acc)
    assert run_schedule(r, which, acc, 3, [None, None, None]) == 8
    r.close()


@pytest.mark.parametrize("acc", ACCS)
def test_odd_even_and_multiple_of_four_chunks(gpu, acc):
    """Steps of 1, 2, 4 and 1 (step_spp 4): k_accumulate's odd, even and multiple-of-4 paths
    at s0 = 0, 1, 3 and 7. Then one step of 8 on a workspace sized for 3: the library runs it
    in pieces of at most 3."""
    r = renderer("cornell", acc)
    assert run_schedule(r, "cornell", acc, 4, [1, 2, 4, 1]) == 8
    with r.progressive(3) as s:
        s.step(8)
        assert s.done == 8 and s.stats["chunk_spp"] <= 3
        ref, ref_stats = oracle_at("cornell", 8)[acc]
        assert_bitwise(s.snapshot(), ref, s.stats, ref_stats)
    r.close()


# ---- 2. launch variants
@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("tune", [{"chunk_units": 3000}, {"slots": 3000}, {"flags": N.TUNE_NO_TAIL}])
def test_launch_variants(gpu, tune, acc):
    """Several chunks per step, few slots (refills), no k_tail; pbr's 600 pixels leave
    k_resolve a partial block."""
    for which in ("glass_spectral", "pbr"):
        r = renderer(which, acc, tuning=N.tuning(**tune))
        run_schedule(r, which, acc, 3, [None, None, None])
        r.close()


# ---- 3. snapshots do not touch the sums
def test_snapshots_leave_the_sums_alone(gpu):
    acc = N.ACC_FORWARD
    r = renderer("glass_spectral", acc)
    with r.progressive(3) as s:
        finals = []
        for _ in range(3):
            s.step()
            a, b = s.snapshot(), s.snapshot(N.SNAP_DISPLAY)
            assert s.snapshot().tobytes() == a.tobytes()
            assert s.snapshot(N.SNAP_DISPLAY).tobytes() == b.tobytes()
        finals.append(s.snapshot())
    with r.progressive(3) as s:  # snapshotted at the end only
        for _ in range(3):
            s.step()
        finals.append(s.snapshot())
        stats = s.stats
    assert finals[0].tobytes() == finals[1].tobytes()
    ref, ref_stats = oracle_at("glass_spectral", 8)[acc]
    assert_bitwise(finals[1], ref, stats, ref_stats)
    r.close()


# ---- 4. tiles and the packed layout
def test_tiles_packed(gpu):
    """Two 16x16 tiles, IZPI_OUT_PACKED, steps 2 and 2: tile after tile, each by sample row y
    then x, holding the oracle's tile render (whose canvas has pixel (x, y) in row H - y)."""
    which, acc = "cornell", N.ACC_RECURSIVE
    _, W, H, _, _ = scene_of(which)
    tiles = ((0, 1, 15, 16), (16, 16, 31, 31))
    r = renderer(which, acc)
    with r.progressive(2, total=4, tiles=np.array(tiles, np.uint32), layout=N.OUT_PACKED) as s:
        for done in (2, 4):
            s.step()
            ref, ref_stats = oracle_at(which, done, tiles)[acc]
            want = np.concatenate([ref[H - y, x0:x1 + 1] for x0, y0, x1, y1 in tiles for y in range(y0, y1 + 1)])
            got = s.snapshot()
            assert got.shape == (2 * 16 * 16 * 4,)
            assert_bitwise(got.reshape(-1, 4), want, s.stats, ref_stats)
    r.close()


# ---- 5. post-processing
def test_post_on_every_snapshot(gpu):
    """POST_SPECTRAL | POST_GAMMA_CLAMP: each snapshot is the oracle's XYZ at spp = done
    through FireflyRejection, XYZToRGB, Gamma and Clamp(1.0)."""
    which, acc = "glass_spectral", N.ACC_RECURSIVE
    _, W, H, _, _ = scene_of(which)
    r = renderer(which, acc)
    with r.progressive(3, post=N.POST_SPECTRAL | N.POST_GAMMA_CLAMP) as s:
        for _ in range(3):
            s.step()
            xyz, ref_stats = oracle_at(which, s.done)[acc]
            rgb = O.xyz_to_rgb(O.firefly(xyz.reshape(-1), W, H), W, H, r.exposure)
            want = O.postprocess(rgb, W, H, [(N.FILTER_GAMMA, 0.0), (N.FILTER_CLAMP, 1.0)]).reshape(H, W, 4)
            assert_bitwise(s.snapshot(), want, s.stats, ref_stats)
    r.close()


# ---- 6. the DISPLAY form
@pytest.mark.parametrize("which", ["cornell", "glass_spectral"])
def test_display_form(gpu, which):
    """Colour: the CANVAS pixels as B, G, R, 1. Spectral: XYZToACEScg of the exposed XYZ
    (no FireflyRejection), as B, G, R, 1."""
    acc = N.ACC_RECURSIVE
    _, W, H, _, sampler = scene_of(which)
    r = renderer(which, acc)
    with r.progressive(3) as s:
        for _ in range(2):
            s.step()
            canvas, shown = s.snapshot(), s.snapshot(N.SNAP_DISPLAY)
            ref, ref_stats = oracle_at(which, s.done)[acc]
            assert_bitwise(canvas, ref, s.stats, ref_stats)
            if sampler == N.SAMPLER_SPECTRAL:
                canvas = O.xyz_to_rgb(canvas.reshape(-1), W, H, r.exposure).reshape(H, W, 4)
                assert (canvas[..., :3] != ref[..., :3]).any()
            assert_bitwise(shown, np.ascontiguousarray(canvas[..., [2, 1, 0, 3]]), s.stats, ref_stats)
    r.close()


# ---- 7. the preview samplers
PAPER, INK = (0.1, 0.2, 0.3), (1.0, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def preview_reference(spp):
    return PR.PreviewRef(configs.cornell_rgb(), 32, 32, spp)


@pytest.mark.parametrize("sampler", [N.SAMPLER_NORMAL, N.SAMPLER_ALBEDO, N.SAMPLER_WIREFRAME])
def test_preview_samplers(gpu, sampler):
    """32x32, N = 4, steps 1 and 3 against the numpy restatement at spp 1 and 4."""
    r = GPURenderer(configs.cornell_rgb(), 32, 32, 4, sampler=sampler, background=PAPER, ink=INK, bvh="gpu")
    with r.progressive(3) as s:
        for n in (1, 3):
            s.step(n)
            want = preview_reference(s.done).render(sampler, PAPER, INK)
            img = s.snapshot()
            assert s.stats["rays"] == s.stats["samples"] == 32 * 32 * s.done
            assert img.tobytes() == want.tobytes(), "max |diff| %g" % np.nanmax(np.abs(img - want))
            shown = s.snapshot(N.SNAP_DISPLAY)
            assert shown.tobytes() == np.ascontiguousarray(img[..., [2, 1, 0, 3]]).tobytes()
    r.close()


# ---- 8. session rules
def test_session_rules(gpu):
    which, acc = "cornell", N.ACC_FORWARD
    _, W, H, _, _ = scene_of(which)
    L = N.lib()
    r = renderer(which, acc)
    canvas = np.zeros((H, W, 4))
    ptr = canvas.ctypes.data_as(C.c_void_p)
    st = N.RenderStats()
    assert L.izpi_gpu_progressive_step(r.ctx, 1, None) == N.IZPI_ERR_INVALID  # no session yet
    assert L.izpi_gpu_progressive_end(r.ctx) == N.IZPI_ERR_INVALID
    s = r.progressive(3)
    assert r.progress() == (0, W * H * 8)
    assert L.izpi_gpu_progressive_snapshot(r.ctx, N.SNAP_CANVAS, ptr) == N.IZPI_ERR_INVALID  # done == 0
    req = r.request()
    assert L.izpi_gpu_progressive_begin(r.ctx, C.byref(req), 3) == N.IZPI_ERR_INVALID  # a second begin
    s.step()
    assert r.progress() == (W * H * 3, W * H * 8)
    # a one-shot render, a prepare and a scene upload are refused and leave the session intact
    rc = L.izpi_gpu_render(r.ctx, C.byref(req), canvas.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
    assert rc == N.IZPI_ERR_INVALID and b"progressive session" in L.izpi_gpu_last_error(r.ctx)
    assert L.izpi_gpu_prepare(r.ctx, C.byref(req)) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_upload_scene(r.ctx, C.byref(r.host.desc)) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_progressive_snapshot(r.ctx, 7, ptr) == N.IZPI_ERR_INVALID  # an unknown form
    assert not canvas.any()
    assert r.progress() == (W * H * 3, W * H * 8)
    s.step()
    ref, ref_stats = oracle_at(which, 6)[acc]
    assert_bitwise(s.snapshot(), ref, s.stats, ref_stats)
    s.step()
    assert s.done == 8
    ref, ref_stats = oracle_at(which, 8)[acc]
    assert_bitwise(s.snapshot(), ref, s.stats, ref_stats)
    s.step()  # at done == N: a no-op
    assert s.done == 8 and r.progress() == (W * H * 8, W * H * 8)
    assert_bitwise(s.snapshot(), ref, s.stats, ref_stats)
    s.close()
    s.close()  # (idempotent)
    assert_bitwise(r.render(), ref, r.stats, ref_stats)  # a one-shot render after end
    with r.progressive(3) as s:  # closed after 3 of 8 samples: cancelled
        s.step()
    assert_bitwise(r.render(), ref, r.stats, ref_stats)
    r.close()


def test_multi_session_rules(gpu):
    """What a device group's session refuses: the status and the exact izpi_gpu_multi_last_error
    text of each call, on two contexts of device 0 and one 16x16 frame."""
    scene = scene_of("cornell")[0]
    L = N.lib()
    m = MultiGPURenderer(scene, 16, 16, 4, [0, 0], bvh="reference")
    req = make_request(16, 16, 4, m.max_depth, m.sampler, m.background, m.seed, m.exposure)
    canvas = np.zeros((16, 16, 4))
    ptr = canvas.ctypes.data_as(C.c_void_p)
    st = (N.RenderStats * 2)()
    ns = N.NoiseStats()
    bad = N.noise_params(threshold=0.0)  # nz::check_params' first rule

    def refused(rc, text):
        assert rc == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_multi_last_error(m.m).decode() == text

    # no session is open
    closed = "no progressive session is open"
    refused(L.izpi_gpu_multi_progressive_step(m.m, 1, st), closed)
    refused(L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_CANVAS, ptr), closed)
    refused(L.izpi_gpu_multi_progressive_noise(m.m, None, C.byref(ns)), closed)
    refused(L.izpi_gpu_multi_progressive_converge(m.m, None, st, C.byref(ns)), closed)
    refused(L.izpi_gpu_multi_progressive_end(m.m), closed)
    # begin
    refused(L.izpi_gpu_multi_progressive_begin(m.m, C.byref(req), 0), "progressive_begin: a request and step_spp >= 1")
    refused(L.izpi_gpu_multi_progressive_begin_ex(m.m, C.byref(req), 2, 2), "progressive_begin: unknown flags")
    refused(L.izpi_gpu_multi_progressive_end(m.m), closed)  # (neither opened one)
    # a session begun without IZPI_PROG_NOISE
    with m.progressive(2) as s:
        refused(L.izpi_gpu_multi_progressive_begin(m.m, C.byref(req), 2), "a progressive session is already open")
        refused(L.izpi_gpu_multi_render(m.m, C.byref(req), ptr, st), "a progressive session is open")
        refused(L.izpi_gpu_multi_prepare(m.m, C.byref(req)), "a progressive session is open")
        refused(L.izpi_gpu_multi_progressive_snapshot(m.m, 7, ptr), "unknown snapshot form")
        first = "snapshot before the session's first sample"
        refused(L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_CANVAS, ptr), first)
        refused(L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_NOISE, ptr), first)  # (before the noise rules)
        assert s.step() == 2
        without = "noise: the session was begun without IZPI_PROG_NOISE"
        refused(L.izpi_gpu_multi_progressive_noise(m.m, None, C.byref(ns)), without)
        refused(L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_NOISE, ptr), without)
        refused(L.izpi_gpu_multi_progressive_converge(m.m, None, st, C.byref(ns)), without)
        # (the parameters come before the session's noise rules)
        refused(L.izpi_gpu_multi_progressive_noise(m.m, C.byref(bad), C.byref(ns)),
                "noise: threshold must be finite and greater than 0")
        assert not canvas.any()
        assert s.done == 2 and m.progress() == (16 * 16 * 2, 16 * 16 * 4)  # the session is intact
        assert s.snapshot().any()
    # a session begun with it
    with m.progressive(1, noise=True) as s:
        assert s.step() == 1
        few = "noise: needs at least 2 samples"
        refused(L.izpi_gpu_multi_progressive_noise(m.m, None, C.byref(ns)), few)
        refused(L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_NOISE, ptr), few)
        refused(L.izpi_gpu_multi_progressive_converge(m.m, C.byref(bad), st, C.byref(ns)),
                "noise: threshold must be finite and greater than 0")
        assert s.done == 1 and m.progress() == (16 * 16, 16 * 16 * 4)
        assert s.step() == 2
        assert s.noise()["done"] == 2
    refused(L.izpi_gpu_multi_progressive_end(m.m), closed)
    m.close()


# ---- 9. multi-GPU
def test_multi_two_contexts_against_the_oracle(gpu):
    which, acc = "cornell", N.ACC_FORWARD
    scene, W, H, spp, sampler = scene_of(which)
    m = MultiGPURenderer(scene, W, H, spp, [0, 0], sampler=sampler, bvh="reference", accumulation=acc)
    with m.progressive(4) as s:
        for n in (2, 2, 4):
            s.step(n)
            ref, ref_stats = oracle_at(which, s.done)[acc]
            total = {k: sum(d[k] for d in s.stats) for k in ref_stats if k in s.stats[0]}  # (the two shares' counters)
            assert_bitwise(s.snapshot(), ref, total, ref_stats)
            assert m.progress() == (W * H * s.done, W * H * 8)
        canvas = s.snapshot()
        shown = s.snapshot(N.SNAP_DISPLAY)
        assert shown.tobytes() == np.ascontiguousarray(canvas[..., [2, 1, 0, 3]]).tobytes()
        with pytest.raises(RuntimeError, match="progressive session"):
            m.render()
    assert m.render().tobytes() == canvas.tobytes()
    m.close()


def test_multi_eight_contexts_equal_the_one_shot(gpu):
    """Eight contexts at 64x64 (quarter-tile units): the final snapshot is
    MultiGPURenderer.render()'s canvas at the same spp, Render's spectral post included."""
    scene, _, _, _, sampler = scene_of("glass_spectral")
    m = MultiGPURenderer(scene, 64, 64, 4, [0] * 8, sampler=sampler, bvh="reference", accumulation=N.ACC_FORWARD)
    with m.progressive(3, post=N.POST_SPECTRAL) as s:
        s.step()
        s.step()
        assert s.done == 4
        got = s.snapshot()
    assert got.tobytes() == m.render(post=N.POST_SPECTRAL).tobytes()
    m.close()


# ---- 10. the command-line tool
def test_cli_progressive(gpu, tmp_path):
    cli = ROOT / "izpi_amd" / "_lib" / "izpi-render"
    example = ROOT / "izpi_amd" / "data" / "scenes" / "cornell_box_transparent_pyramid_spectral.pbtxt"
    base = [str(cli), "--scene", str(example), "--x", "64", "--y", "64", "--samples", "4"]
    one, prog, prefix = tmp_path / "one.pfm", tmp_path / "prog.pfm", tmp_path / "snap"
    for extra in (["--out", str(one)], ["--out", str(prog), "--progressive", "1", "--snapshots", str(prefix)]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    assert one.read_bytes() == prog.read_bytes()
    snaps = [Path("%s_%d.pfm" % (prefix, k)) for k in (1, 2, 3, 4)]
    assert all(p.exists() for p in snaps)
    assert snaps[3].read_bytes() == one.read_bytes()
    assert snaps[0].read_bytes() != one.read_bytes()
