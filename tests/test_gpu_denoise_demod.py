"""Albedo demodulation of the two a-trous denoisers on the GPU (IZPI_DENOISE_DEMODULATE;
k_demodulate, k_remodulate, izpi_amd/csrc/denoise.hip): to the byte
against the host twins, which tests/test_denoise_demod.py ties to the Python restatement without
a GPU, through the host-pointer and the device entries; flagged and unflagged calls alternating
on one context's scratch; GPURenderer.render_denoised and ProgressiveSession.denoised with
demodulate=True on a textured scene; and the command-line tool."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import build, configs
from izpi_amd.renderer import (GPURenderer, denoise, denoise_device, denoise_var, denoise_var_device, host_denoise,
                               host_denoise_var)
from tests import adapt_ref as AR
from tests import denoise_demod_ref as MR
from tests import noise_ref as NR
from tests.test_denoise_demod import textured_lambert_box

pytestmark = pytest.mark.gpu

FIXED, GUIDED = N.denoise_params(demodulate=True), N.denoise_var_params(demodulate=True)


@pytest.fixture(scope="module")
def ctx(gpu):
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    yield h
    N.lib().izpi_gpu_close(h)


def assert_same(got, want):
    """Bit-identical arrays (a NaN matches a NaN of the same bits)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "max |diff| %g at %d doubles" % (
        np.nanmax(np.abs(got - want)), int((got.view(np.uint64) != want.view(np.uint64)).sum()))


@functools.lru_cache(maxsize=None)
def big():
    """261 x 67 seeded frames (many blocks, ragged edges) with every special texel and pixel of
    denoise_demod_ref.seeded (read only)."""
    return MR.seeded(261, 67, seed=3)


@functools.lru_cache(maxsize=None)
def big_twin(var, demodulate=True):
    c, S, nm, al = big()
    if var:
        return host_denoise_var(c, S, nm, al, N.denoise_var_params(demodulate=demodulate))
    return host_denoise(c, nm, al, N.denoise_params(demodulate=demodulate))


def on_device(gpu, frames, shape):
    import torch
    dev = torch.device("cuda", gpu)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    out = torch.zeros(shape, dtype=torch.float64, device=dev)
    var = torch.zeros(shape[:2], dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    return d, out, var


# ------------------------------------------------ 1. the device == the twin, both kinds of entry
@pytest.mark.parametrize("case", MR.cases(), ids=MR.case_id)
def test_device_equals_the_twin_bytewise(ctx, gpu, case):
    w, h, n, guides = case
    c, S, nm, al = MR.seeded(w, h)
    keep = [f.copy() for f in (c, S, al)]
    nm, al = MR.pick_guides(nm, al, guides)
    fixed, guided = N.denoise_params(iterations=n, demodulate=True), N.denoise_var_params(iterations=n, demodulate=True)
    want = host_denoise(c, nm, al, fixed)
    want_g, want_var = host_denoise_var(c, S, nm, al, guided)
    # the host-pointer entries
    timing = {}
    assert_same(denoise(ctx, c, nm, al, fixed, timing=timing), want)
    assert timing["ms"] > 0
    got, var = denoise_var(ctx, c, S, nm, al, guided)
    assert_same(got, want_g)
    assert_same(var, want_var)
    # the device entries
    d, out, dvar = on_device(gpu, (c, S, al) + (() if nm is None else (nm,)), (h, w, 4))
    nm_ptr = None if nm is None else d[3].data_ptr()
    assert denoise_device(ctx, d[0].data_ptr(), nm_ptr, d[2].data_ptr(), out.data_ptr(), w, h, fixed) > 0
    assert_same(out.cpu().numpy(), want)
    denoise_var_device(ctx, d[0].data_ptr(), d[1].data_ptr(), nm_ptr, d[2].data_ptr(), out.data_ptr(), dvar.data_ptr(), w, h,
                       guided)
    assert_same(out.cpu().numpy(), want_g)
    assert_same(dvar.cpu().numpy(), want_var)
    for t, f in zip(d, (c, S, al)):
        assert_same(t.cpu().numpy(), f)  # the device inputs are unchanged
    for f, k in zip((c, S, al), keep):
        assert_same(f, k)  # ... and the host ones


def test_many_blocks_equal_the_twin_through_both_kinds_of_entry(ctx, gpu):
    width, height = 261, 67
    frames = big()
    c, S, nm, al = frames
    assert_same(denoise(ctx, c, nm, al, FIXED), big_twin(False))
    got, var = denoise_var(ctx, c, S, nm, al, GUIDED)
    assert_same(got, big_twin(True)[0])
    assert_same(var, big_twin(True)[1])
    d, out, dvar = on_device(gpu, frames, (height, width, 4))
    ptr = [t.data_ptr() for t in d]
    ms = denoise_device(ctx, ptr[0], ptr[2], ptr[3], out.data_ptr(), width, height, FIXED)
    print("%d x %d, 5 iterations demodulated: %.3f ms on the device" % (width, height, ms))
    assert_same(out.cpu().numpy(), big_twin(False))
    denoise_var_device(ctx, *ptr, out.data_ptr(), dvar.data_ptr(), width, height, GUIDED)
    assert_same(out.cpu().numpy(), big_twin(True)[0])
    assert_same(dvar.cpu().numpy(), big_twin(True)[1])
    out.zero_()
    denoise_var_device(ctx, *ptr, out.data_ptr(), None, width, height, GUIDED)  # without a plane: the same canvas
    assert_same(out.cpu().numpy(), big_twin(True)[0])
    for t, f in zip(d, frames):
        assert_same(t.cpu().numpy(), f)


def test_argument_checks_match_the_twin(ctx):
    L = N.lib()
    c, S, al = np.ones((4, 4, 4)), np.full((4, 4, 4), 0.1), np.full((4, 4, 4), 0.5)
    out, var = np.full((4, 4, 4), 7.0), np.full((4, 4), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    floor = N.DENOISE_VAR_DEFAULT_FLOOR
    messages = set()
    for flags, albedo in ((1, al), (2, al), (3, al), (5, al), (8, al), (N.DENOISE_DEMODULATE, None)):
        params = N.denoise_params()
        params.flags = flags
        pp = C.byref(params)
        assert L.izpi_host_denoise(p(c), None, p(albedo), p(out), 4, 4, pp) == N.IZPI_ERR_INVALID
        msg = L.izpi_host_last_error().decode()
        messages.add(msg)
        for entry in (L.izpi_gpu_denoise, L.izpi_gpu_denoise_device):  # refused before any pointer is used
            assert entry(ctx, p(c), None, p(albedo), p(out), 4, 4, pp, None) == N.IZPI_ERR_INVALID
            assert L.izpi_gpu_last_error(ctx).decode() == msg
        for entry in (L.izpi_gpu_denoise_var, L.izpi_gpu_denoise_var_device):
            assert entry(ctx, p(c), p(S), None, p(albedo), p(out), p(var), 4, 4, pp, floor, None) == N.IZPI_ERR_INVALID
            assert L.izpi_gpu_last_error(ctx).decode() == msg
    assert messages == {"denoise: flags must be 0", "denoise: demodulation needs the albedo canvas"}
    assert (out == 7.0).all() and (var == 7.0).all()


# ------------------------------------------------ 2. the scratch buffers grow, are reused and are shared
def test_flagged_and_unflagged_calls_alternate_on_one_context(gpu):
    """One context: a small frame, a large one, the small one again; on each, both filters with
    and without the flag in turn. d_demod, d_denoise and d_dnvar grow and are reused, and every
    call still matches its own twin."""
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    try:
        small = MR.seeded(40, 30)
        want_small = {(v, f): (host_denoise_var(*small, N.denoise_var_params(demodulate=f)) if v else
                               host_denoise(small[0], small[2], small[3], N.denoise_params(demodulate=f)))
                      for v in (False, True) for f in (False, True)}
        want_large = {(v, f): big_twin(v, f) for v in (False, True) for f in (False, True)}
        for frames, want in ((small, want_small), (big(), want_large), (small, want_small)):
            c, S, nm, al = frames
            for flag in (True, False, True):
                assert_same(denoise(h, c, nm, al, N.denoise_params(demodulate=flag)), want[(False, flag)])
                got, var = denoise_var(h, c, S, nm, al, N.denoise_var_params(demodulate=flag))
                assert_same(got, want[(True, flag)][0])
                assert_same(var, want[(True, flag)][1])
    finally:
        N.lib().izpi_gpu_close(h)


# ------------------------------------------------ 3. render_denoised
def test_render_denoised_demodulated_equals_the_twin_of_the_three_frames(gpu):
    scene = textured_lambert_box()
    frames = []
    for sampler in (N.SAMPLER_COLOUR, N.SAMPLER_NORMAL, N.SAMPLER_ALBEDO):  # each by a renderer of its own, all at 8 spp
        r = GPURenderer(scene, 40, 30, 8, sampler=sampler, bvh="gpu", accumulation=N.ACC_FORWARD)
        frames.append(r.render())
        r.close()
    colour, normal, albedo = frames
    want = host_denoise(colour, normal, albedo, FIXED)
    assert want.tobytes() != host_denoise(colour, normal, albedo).tobytes()
    r = GPURenderer(scene, 40, 30, 8, bvh="gpu", accumulation=N.ACC_FORWARD)
    got = r.render_denoised(demodulate=True, post=N.POST_GAMMA_CLAMP)  # the guides at the frame's 8 spp
    live = want[..., 3] != 0
    post = want.copy()
    post[..., :3] = np.minimum(np.sqrt(want[..., :3]), 1.0)
    assert np.array_equal(got[live], post[live]) and r.sampler == N.SAMPLER_COLOUR
    assert_same(r.last_noisy, colour)
    assert_same(r.render_denoised(demodulate=True), want)
    # the caller's params keep their values and gain the flag; the caller's struct is not written
    p = N.denoise_params(iterations=2, sigma_colour=2.0)
    assert_same(r.render_denoised(params=p, demodulate=True),
                host_denoise(colour, normal, albedo, N.denoise_params(iterations=2, sigma_colour=2.0, demodulate=True)))
    assert p.flags == 0
    with pytest.raises(ValueError, match="Albedo"):
        r.render_denoised(demodulate=True, albedo=False)
    r.close()


def test_render_denoised_demodulated_refuses_the_spectral_sampler(gpu):
    r = GPURenderer(configs.cornell_glass_spectral(40 / 30), 40, 30, 4, sampler=N.SAMPLER_SPECTRAL, bvh="gpu")
    with pytest.raises(ValueError, match="Colour sampler"):
        r.render_denoised(demodulate=True)
    r.close()


# ------------------------------------------------ 4. a noise session
W, H, CAP = 40, 30, 8


@functools.lru_cache(maxsize=None)
def textured_canvases():
    return tuple(NR.sample_canvases(textured_lambert_box(), W, H, CAP, N.SAMPLER_COLOUR, N.ACC_FORWARD))


def mean_canvas(canvases, n):
    s, _ = NR.fold(canvases, n)
    c = np.zeros(canvases[0].shape)
    c[..., :3] = NR.mean_of(s, n, N.SAMPLER_COLOUR)
    c[..., 3] = canvases[0][..., 3]
    return c


def test_a_noise_session_denoised_demodulated_equals_the_twin_of_its_snapshots(gpu):
    """textured_lambert_box 40 x 30, forward accumulation, steps of 1, 2, 4, 1 with the guides at
    the session's cap: from done = 3 on the filtered frame is the twin's over the numpy reference
    of the two snapshots, the session's own snapshots stay the reference's, and stepping on
    reaches the uninterrupted session's canvas."""
    canvases = textured_canvases()
    r = GPURenderer(textured_lambert_box(), W, H, CAP, accumulation=N.ACC_FORWARD)
    whole = r.render()
    guides = r.render_guides(aov_spp=CAP)
    normal, albedo = (g.cpu().numpy() for g in guides)
    filtered = 0
    with r.progressive(4, noise=True) as s:
        s.step(1)
        for k in (2, 4, 1):
            s.step(k)
            colour = mean_canvas(canvases, s.done)
            se = NR.reference(canvases, s.done, W, H, N.SAMPLER_COLOUR)[0]
            got, var = s.denoised(guides, demodulate=True)
            want, want_var = host_denoise_var(colour, se, normal, albedo, GUIDED)
            assert_same(got, want)
            assert_same(var, want_var)
            assert got.tobytes() != colour.tobytes() and s.denoise_ms > 0
            assert got.tobytes() != host_denoise_var(colour, se, normal, albedo)[0].tobytes()
            assert_same(s.snapshot(), colour)
            assert_same(s.snapshot(N.SNAP_NOISE), se)
            filtered += 1
        assert s.done == CAP and filtered == 3
        assert_same(s.snapshot(), whole)  # the uninterrupted frame
        # the caller's params gain the flag; guides without an albedo are refused
        p = N.denoise_params(2, 3.0, 0.25, 1.0)
        got, var = s.denoised(guides, p, 1e-3, demodulate=True)
        want, want_var = host_denoise_var(colour, se, normal, albedo, N.denoise_params(2, 3.0, 0.25, 1.0, demodulate=True), 1e-3)
        assert_same(got, want)
        assert_same(var, want_var)
        assert p.flags == 0
        with pytest.raises(ValueError, match="Albedo"):
            s.denoised((guides[0], None), demodulate=True)
    r.close()


def test_an_adaptive_session_denoised_demodulated_equals_the_twin_of_its_snapshots(gpu, monkeypatch):
    """The same scene, threshold 0.25, steps of 2 with adapt after each: adapt_ref simulates the
    session over its named cases, so the textured box is given to it under a name of its own."""
    from tests import test_forward_accumulation as FA
    named = FA.scene_case
    monkeypatch.setattr(FA, "scene_case", lambda which: (textured_lambert_box(), W, H, CAP, N.SAMPLER_COLOUR)
                        if which == "textured_lambert" else named(which))
    steps = (2,) * 4
    rule = dict(threshold=0.25, floor=0.01, tolerated=0.05, min_spp=2)
    ref, w, h, _ = AR.simulate("textured_lambert", N.ACC_FORWARD, list(steps), rule, size=(W, H), counters=False)
    assert (w, h) == (W, H) and len(set(ref[-1]["n"][ref[-1]["counted"]].tolist())) >= 2  # several distinct n_p
    r = GPURenderer(textured_lambert_box(), W, H, CAP, accumulation=N.ACC_FORWARD)
    guides = r.render_guides(aov_spp=CAP)
    normal, albedo = (g.cpu().numpy() for g in guides)
    with r.progressive(2, total=CAP, noise=True, adaptive=True) as s:
        for k, st in zip(steps, ref):
            s.step(k)
            assert s.adapt(**rule)["active"] == st["adapt"]["active"]
            canvas, var = s.denoised(guides, demodulate=True)
            want, want_var = host_denoise_var(st["canvas"], st["noise"], normal, albedo, GUIDED)
            assert_same(canvas, want)
            assert_same(var, want_var)
            assert_same(s.snapshot(), st["canvas"])
            assert_same(s.snapshot(N.SNAP_NOISE), st["noise"])
    r.close()


# ------------------------------------------------ 5. the command-line tool
def test_cli_denoise_demodulate_writes_the_twin_s_frames(gpu, tmp_path):
    scene = configs.cornell_rgb(W / H)
    frames = []
    for sampler in (N.SAMPLER_COLOUR, N.SAMPLER_NORMAL, N.SAMPLER_ALBEDO):  # the guides at --samples, not at 4
        r = GPURenderer(scene, W, H, 8, sampler=sampler, bvh="gpu", accumulation=N.ACC_FORWARD)
        frames.append(r.render())
        r.close()
    colour, normal, albedo = frames
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(W / H))
    raw, vpfm = tmp_path / "d.f64", tmp_path / "v.pfm"
    base = [str(build.CLI), "--scene", str(box), "--x", str(W), "--y", str(H), "--samples", "8", "--raw", str(raw)]
    run = subprocess.run(base + ["--denoise", "--denoise-demodulate"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "denoised (demodulated), 5 iterations" in run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(H, W, 4), host_denoise(colour, normal, albedo, FIXED))
    # the variance-guided filter over a session's frame
    r = GPURenderer(scene, W, H, 8, bvh="gpu", accumulation=N.ACC_FORWARD)
    with r.progressive(4, noise=True) as s:
        s.step()
        s.step()
        assert_same(s.snapshot(), colour)
        want, want_var = host_denoise_var(colour, s.snapshot(N.SNAP_NOISE), normal, albedo, GUIDED)
    r.close()
    session = ["--progressive", "4", "--noise-threshold", "0.0001"]  # (never met: the frame has all 8 samples)
    run = subprocess.run(base + session + ["--denoise-variance", "--denoise-demodulate", "--variance-out", str(vpfm)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stderr.splitlines() if ln.startswith("IZPI_DENOISE_VAR ")]
    assert len(lines) == 1 and lines[0].endswith(" demodulated"), run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(H, W, 4), want)
    head = b"PF\n40 30\n-1.0\n"
    data = vpfm.read_bytes()
    assert data.startswith(head)
    pixels = np.frombuffer(data[len(head):], "<f4").reshape(H, W, 3)[::-1]  # bottom row first
    assert np.array_equal(pixels, np.repeat(want_var[..., None], 3, 2).astype(np.float32))
    # alone, or on a spectral frame, the option is refused
    run = subprocess.run(base + ["--denoise-demodulate"], capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "--denoise-demodulate needs --denoise or --denoise-variance" in run.stderr
    run = subprocess.run(base + ["--sampler", "spectral", "--denoise", "--denoise-demodulate"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode != 0 and "--denoise-demodulate needs --sampler colour" in run.stderr
