"""The edge-avoiding a-trous denoiser on the GPU (izpi_gpu_denoise, izpi_gpu_denoise_device,
izpi_amd/csrc/denoise.hip): to the byte against the host twin
(izpi_host_denoise), which tests/test_denoise.py ties to the Python restatement without a GPU;
the context's scratch canvas; GPURenderer.render_denoised against the three frames rendered
separately; a progressive session left intact; and the command-line tool."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import build, configs
from izpi_amd.renderer import GPURenderer, denoise, denoise_device, host_denoise
from tests import denoise_ref as DR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    yield h
    N.lib().izpi_gpu_close(h)


@functools.lru_cache(maxsize=None)
def big(width, height):
    """Seeded frames spanning many blocks, with a dead row 0, a NaN and an Inf pixel (read only)."""
    c, nm, al = DR.seeded(width, height, seed=3, variant="dead_row0")
    c[height // 2, width // 3, 1] = float("nan")
    c[height // 3, width // 2, 2] = float("inf")
    return c, nm, al


@functools.lru_cache(maxsize=None)
def twin(width, height, iterations):
    return host_denoise(*big(width, height), N.denoise_params(iterations=iterations))


def assert_same(got, want):
    assert got.tobytes() == want.tobytes(), "max |diff| %g at %d doubles" % (
        np.nanmax(np.abs(got - want)), int((got.view(np.uint64) != want.view(np.uint64)).sum()))


# ------------------------------------------------ 1. the device == the twin, small cases
@pytest.mark.parametrize("case", DR.cases(), ids=DR.case_id)
def test_device_equals_the_twin_bytewise(ctx, case):
    w, h, variant, n, guides = case
    c, nm, al = DR.seeded(w, h, variant=variant)
    nm, al = DR.pick_guides(nm, al, guides)
    p = N.denoise_params(iterations=n)
    timing = {}
    got = denoise(ctx, c, nm, al, p, timing=timing)
    assert_same(got, host_denoise(c, nm, al, p))
    assert timing["ms"] > 0


# ------------------------------------------------ 2. many blocks, ragged edges, device pointers
@pytest.mark.parametrize("width,height,iterations", [(256, 256, 5), (261, 67, 5), (256, 256, 8)])
def test_device_entry_equals_the_twin_on_many_blocks(ctx, gpu, width, height, iterations):
    import torch
    dev = torch.device("cuda", gpu)
    frames = big(width, height)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    out = torch.zeros((height, width, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ms = denoise_device(ctx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), width, height,
                        N.denoise_params(iterations=iterations))
    torch.cuda.synchronize(dev)
    print("%d x %d, %d iterations: %.3f ms on the device" % (width, height, iterations, ms))
    assert ms > 0
    assert_same(out.cpu().numpy(), twin(width, height, iterations))
    for t, f in zip(d, frames):
        assert t.cpu().numpy().tobytes() == f.tobytes()  # the inputs are unchanged


def test_argument_checks_match_the_twin(ctx):
    L = N.lib()
    c = np.ones((4, 4, 4))
    out = np.full((4, 4, 4), 7.0)
    bad = N.denoise_params(iterations=9)
    for args in ((c, c, 4, 4, None), (c, out, 4, 4, bad), (c, out, 0, 4, None),
                 (c, out, 4, 4, N.denoise_params(sigma_colour=0.0)), (c, out, 4, 4, N.denoise_params(sigma_albedo=float("nan")))):
        a, o, w, h, p = args
        pp = None if p is None else C.byref(p)
        host_rc = L.izpi_host_denoise(a.ctypes.data_as(C.c_void_p), None, None, o.ctypes.data_as(C.c_void_p), w, h, pp)
        host_msg = L.izpi_host_last_error().decode()
        for entry in (L.izpi_gpu_denoise, L.izpi_gpu_denoise_device):  # refused before any pointer is used
            rc = entry(ctx, a.ctypes.data_as(C.c_void_p), None, None, o.ctypes.data_as(C.c_void_p), w, h, pp, None)
            assert rc == host_rc == N.IZPI_ERR_INVALID
            assert L.izpi_gpu_last_error(ctx).decode() == host_msg and host_msg.startswith("denoise: ")
    assert (out == 7.0).all()


# ------------------------------------------------ 3. the scratch canvas grows and is reused
def test_scratch_grows_and_is_reused(gpu):
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    try:
        small = DR.seeded(40, 30, variant="dead_row0")
        want_small = host_denoise(*small)
        for frames, want in ((small, want_small), (big(256, 256), twin(256, 256, 5)), (small, want_small)):
            assert_same(denoise(h, *frames), want)
    finally:
        N.lib().izpi_gpu_close(h)


# ------------------------------------------------ 4. render_denoised
def _frames(scene, sampler, acc, spp, aov_spp, albedo):
    """The three frames rendered separately, each by a renderer of its own."""
    out = []
    for s, n, post in ((sampler, spp, N.POST_SPECTRAL if sampler == N.SAMPLER_SPECTRAL else N.POST_NONE),
                       (N.SAMPLER_NORMAL, aov_spp, N.POST_NONE), (N.SAMPLER_ALBEDO, aov_spp, N.POST_NONE)):
        if s == N.SAMPLER_ALBEDO and not albedo:
            out.append(None)
            continue
        r = GPURenderer(scene, 40, 30, n, sampler=s, bvh="gpu", accumulation=acc)
        out.append(r.render(post=post))
        r.close()
    return out


@functools.lru_cache(maxsize=None)
def cornell_frames(acc):
    return _frames(configs.cornell_rgb(40 / 30), N.SAMPLER_COLOUR, acc, 4, 4, True)


def test_render_denoised_equals_the_twin_of_the_three_frames(gpu):
    colour, normal, albedo = cornell_frames(N.ACC_RECURSIVE)
    want = host_denoise(colour, normal, albedo)
    assert want.tobytes() != colour.tobytes()
    r = GPURenderer(configs.cornell_rgb(40 / 30), 40, 30, 4, bvh="gpu")
    before = r.render()
    assert_same(before, colour)
    got = r.render_denoised(aov_spp=4)
    assert_same(got, want)
    assert_same(r.last_noisy, colour)
    assert r.denoise_ms > 0 and r.sampler == N.SAMPLER_COLOUR
    assert r.stats["samples"] == 40 * 30 * 4
    # Gamma and Clamp come after the filter, on its output
    got = r.render_denoised(post=N.POST_GAMMA_CLAMP)
    live = want[..., 3] != 0
    post = want.copy()
    post[..., :3] = np.minimum(np.sqrt(want[..., :3]), 1.0)
    assert np.array_equal(got[live], post[live]) and r.sampler == N.SAMPLER_COLOUR
    # other parameters reach the filter, and the renderer renders as before
    p = N.denoise_params(iterations=2, sigma_colour=2.0)
    assert_same(r.render_denoised(params=p), host_denoise(colour, normal, albedo, p))
    assert_same(r.render_denoised(albedo=False), host_denoise(colour, normal, None))
    assert_same(r.render(), before)
    r.close()


def test_render_denoised_spectral_uses_the_normal_guide_only(gpu):
    scene = configs.cornell_glass_spectral(40 / 30)
    colour, normal, _ = _frames(scene, N.SAMPLER_SPECTRAL, N.ACC_RECURSIVE, 4, 4, False)
    r = GPURenderer(scene, 40, 30, 4, sampler=N.SAMPLER_SPECTRAL, bvh="gpu")
    got = r.render_denoised()
    assert_same(got, host_denoise(colour, normal, None))
    assert_same(r.last_noisy, colour)
    assert r.sampler == N.SAMPLER_SPECTRAL
    assert_same(r.render(post=N.POST_SPECTRAL), colour)
    r.close()


# ------------------------------------------------ 5. beside an open progressive session
def test_denoising_a_snapshot_leaves_the_session_intact(gpu):
    import torch
    dev = torch.device("cuda", gpu)
    r = GPURenderer(configs.cornell_rgb(40 / 30), 40, 30, 8, bvh="gpu")
    with r.progressive(3) as s:
        s.step()
        s.step()
        s.step()
        want = s.snapshot()
    snap = torch.zeros((30, 40, 4), dtype=torch.float64, device=dev)
    out = torch.zeros((30, 40, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    with r.progressive(3) as s:
        s.step()
        s.snapshot_device(snap.data_ptr())
        at3 = s.snapshot()
        assert r.denoise_device(snap.data_ptr(), None, None, out.data_ptr()) > 0
        torch.cuda.synchronize(dev)
        assert_same(snap.cpu().numpy(), at3)
        assert_same(out.cpu().numpy(), host_denoise(at3))
        s.step()
        s.step()
        assert s.done == 8
        assert_same(s.snapshot(), want)
    r.close()


# ------------------------------------------------ 6. the command-line tool
def test_cli_denoise_writes_the_denoised_frame(gpu, tmp_path):
    colour, normal, albedo = cornell_frames(N.ACC_RECURSIVE)  # render_denoised's frames above
    want = host_denoise(colour, normal, albedo)
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(40 / 30))
    raw, pfm = tmp_path / "d.f64", tmp_path / "d.pfm"
    run = subprocess.run([str(build.CLI), "--scene", str(box), "--x", "40", "--y", "30", "--samples", "4", "--denoise",
                          "--accumulation", "recursive", "--raw", str(raw), "--out", str(pfm)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "denoised, 5 iterations" in run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(30, 40, 4), want)
    data = pfm.read_bytes()
    head = b"PF\n40 30\n-1.0\n"
    assert data.startswith(head)
    pixels = np.frombuffer(data[len(head):], "<f4").reshape(30, 40, 3)[::-1]  # bottom row first
    assert np.array_equal(pixels, want[..., :3].astype(np.float32))
    # --denoise N and --denoise-sigma reach the filter; a preview sampler is refused
    run = subprocess.run([str(build.CLI), "--scene", str(box), "--x", "40", "--y", "30", "--samples", "4", "--denoise", "2",
                          "--denoise-sigma", "2,0.25,1", "--accumulation", "recursive", "--raw", str(raw)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(30, 40, 4),
                host_denoise(colour, normal, albedo, N.denoise_params(2, 2.0, 0.25, 1.0)))
    run = subprocess.run([str(build.CLI), "--scene", str(box), "--x", "40", "--y", "30", "--sampler", "normal", "--denoise"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "--denoise needs --sampler colour or spectral" in run.stderr
