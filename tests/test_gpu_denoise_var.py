"""The variance-guided a-trous denoiser on the GPU (izpi_gpu_denoise_var, izpi_gpu_denoise_var_device,
izpi_amd/csrc/denoise.hip): to the byte against the host twin
(izpi_host_denoise_var), which tests/test_denoise_var.py ties to the Python restatement without
a GPU; the context's scratch shared with the filter of section 3.8; ProgressiveSession.denoised
on a plain, an adaptive and a Spectral noise session against the twin applied to the numpy
references of their snapshots (tests/noise_ref.py, tests/adapt_ref.py); and the command-line tool."""
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
from tests import denoise_ref as DR
from tests import denoise_var_ref as VR
from tests import noise_ref as NR
from tests.test_forward_accumulation import scene_case

pytestmark = pytest.mark.gpu


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
def big(width, height):
    """Seeded frames spanning many blocks, with a dead row 0, NaN and Inf pixels in the colour and
    in the standard errors, and a block without variance (read only)."""
    c, S, nm, al = VR.seeded(width, height, seed=3, variant="dead_row0")
    c[height // 2, width // 3, 1] = float("nan")
    c[height // 3, width // 2, 2] = float("inf")
    S[height // 2, width // 3 + 3, 0] = float("nan")
    S[height // 3, width // 2 + 3, 1] = float("inf")
    S[height - 6:height - 2, 5:12, :3] = 0.0
    return c, S, nm, al


@functools.lru_cache(maxsize=None)
def big_twin(width, height, iterations):
    return host_denoise_var(*big(width, height), N.denoise_var_params(iterations=iterations))


# ------------------------------------------------ 1. the device == the twin, small cases
@pytest.mark.parametrize("case", VR.cases(), ids=VR.case_id)
def test_device_equals_the_twin_bytewise(ctx, case):
    w, h, variant, n, guides = case
    c, S, nm, al = VR.seeded(w, h, variant=variant)
    nm, al = DR.pick_guides(nm, al, guides)
    p = N.denoise_var_params(iterations=n)
    timing = {}
    got, var = denoise_var(ctx, c, S, nm, al, p, timing=timing)
    want, want_var = host_denoise_var(c, S, nm, al, p)
    assert_same(got, want)
    assert_same(var, want_var)
    assert timing["ms"] > 0


def test_other_parameters_reach_the_kernel(ctx):
    c, S, nm, al = VR.seeded(37, 19)
    p = N.denoise_params(3, 3.0, 0.25, 1.0)
    got, var = denoise_var(ctx, c, S, nm, al, p, 1e-3)
    want, want_var = host_denoise_var(c, S, nm, al, p, 1e-3)
    assert_same(got, want)
    assert_same(var, want_var)
    assert got.tobytes() != host_denoise_var(c, S, nm, al)[0].tobytes()
    got, var = denoise_var(ctx, c, S, None, al)  # the Albedo guide alone: the fourth instance
    want, want_var = host_denoise_var(c, S, None, al)
    assert_same(got, want)
    assert_same(var, want_var)


# ------------------------------------------------ 2. many blocks, ragged edges, device pointers
def test_device_entry_equals_the_twin_on_many_blocks(ctx, gpu):
    import torch
    width, height, iterations = 261, 67, 5
    dev = torch.device("cuda", gpu)
    frames = big(width, height)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    out = torch.zeros((height, width, 4), dtype=torch.float64, device=dev)
    var = torch.zeros((height, width), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ms = denoise_var_device(ctx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(),
                            var.data_ptr(), width, height, N.denoise_var_params(iterations=iterations))
    torch.cuda.synchronize(dev)
    print("%d x %d, %d iterations: %.3f ms on the device" % (width, height, iterations, ms))
    assert ms > 0
    want, want_var = big_twin(width, height, iterations)
    assert_same(out.cpu().numpy(), want)
    assert_same(var.cpu().numpy(), want_var)
    for t, f in zip(d, frames):
        assert t.cpu().numpy().tobytes() == f.tobytes()  # the inputs are unchanged
    # without a variance output the canvas is the same
    out.zero_()
    torch.cuda.synchronize(dev)
    denoise_var_device(ctx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(), None,
                       width, height, N.denoise_var_params(iterations=iterations))
    assert_same(out.cpu().numpy(), want)


def test_device_entry_without_a_variance_output_equals_the_twin(ctx, gpu):
    """The variance ping-pong's last write: with var_out_ptr=None it lands in a scratch plane,
    with a plane in the caller's. 37 x 19 plain frames, both guides; iterations 0 (a copy),
    1 (no scratch canvas), 2 and 5; then 2 again with a plane."""
    import torch
    width, height = 37, 19
    dev = torch.device("cuda", gpu)
    frames = VR.seeded(width, height)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    out = torch.zeros((height, width, 4), dtype=torch.float64, device=dev)
    var = torch.zeros((height, width), dtype=torch.float64, device=dev)
    ptrs = [t.data_ptr() for t in d]
    for iterations in (0, 1, 2, 5):
        p = N.denoise_var_params(iterations=iterations)
        out.fill_(7.0)
        torch.cuda.synchronize(dev)
        denoise_var_device(ctx, *ptrs, out.data_ptr(), None, width, height, p)
        assert_same(out.cpu().numpy(), host_denoise_var(*frames, p)[0])
    p = N.denoise_var_params(iterations=2)
    out.fill_(7.0)
    var.fill_(7.0)
    torch.cuda.synchronize(dev)
    denoise_var_device(ctx, *ptrs, out.data_ptr(), var.data_ptr(), width, height, p)
    want, want_var = host_denoise_var(*frames, p)
    assert_same(out.cpu().numpy(), want)
    assert_same(var.cpu().numpy(), want_var)


def test_argument_checks_match_the_twin(ctx):
    L = N.lib()
    c = np.ones((4, 4, 4))
    S = np.full((4, 4, 4), 0.1)
    out = np.full((4, 4, 4), 7.0)
    var = np.full((4, 4), 7.0)
    floor = N.DENOISE_VAR_DEFAULT_FLOOR
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for args in ((c, S, c, var, 4, 4, None, floor), (c, S, S, var, 4, 4, None, floor), (c, None, out, var, 4, 4, None, floor),
                 (c, S, out, out.reshape(-1)[:16], 4, 4, None, floor), (c, S, out, var, 4, 4, N.denoise_params(iterations=9), floor),
                 (c, S, out, var, 0, 4, None, floor), (c, S, out, var, 4, 4, N.denoise_params(sigma_colour=0.0), floor),
                 (c, S, out, var, 4, 4, None, 0.0), (c, S, out, var, 4, 4, None, float("nan"))):
        a, s, o, v, w, h, params, fl = args
        pp = None if params is None else C.byref(params)
        host_rc = L.izpi_host_denoise_var(p(a), p(s), None, None, p(o), p(v), w, h, pp, fl)
        host_msg = L.izpi_host_last_error().decode()
        for entry in (L.izpi_gpu_denoise_var, L.izpi_gpu_denoise_var_device):  # refused before any pointer is used
            rc = entry(ctx, p(a), p(s), None, None, p(o), p(v), w, h, pp, fl, None)
            assert rc == host_rc == N.IZPI_ERR_INVALID
            assert L.izpi_gpu_last_error(ctx).decode() == host_msg and host_msg.startswith("denoise: ")
    assert (out == 7.0).all() and (var == 7.0).all()


# ------------------------------------------------ 3. the scratch grows, is reused, and is shared
def test_scratch_grows_is_reused_and_is_shared_with_the_other_filter(gpu):
    """One context: a small frame, a large one, the small one again, each through both filters
    in turn. Both ping-pong through d_denoise; each must still match its own twin."""
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    try:
        small = VR.seeded(40, 30, variant="dead_row0")
        want_small = host_denoise_var(*small)
        old_small = host_denoise(small[0], small[2], small[3])
        large = big(261, 67)
        old_large = host_denoise(large[0], large[2], large[3])
        for frames, want, old in ((small, want_small, old_small), (large, big_twin(261, 67, 5), old_large),
                                  (small, want_small, old_small)):
            got, var = denoise_var(h, *frames)
            assert_same(got, want[0])
            assert_same(var, want[1])
            assert_same(denoise(h, frames[0], frames[2], frames[3]), old)
            got, var = denoise_var(h, *frames)
            assert_same(got, want[0])
            assert_same(var, want[1])
    finally:
        N.lib().izpi_gpu_close(h)


def test_both_device_entries_alternate_on_one_context(ctx, gpu):
    import torch
    width, height = 261, 67
    dev = torch.device("cuda", gpu)
    frames = big(width, height)
    c, S, nm, al = (torch.from_numpy(f).to(dev) for f in frames)
    out = torch.zeros((height, width, 4), dtype=torch.float64, device=dev)
    var = torch.zeros((height, width), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    old = host_denoise(frames[0], frames[2], frames[3])
    want, want_var = big_twin(width, height, 5)
    for _ in range(2):
        denoise_device(ctx, c.data_ptr(), nm.data_ptr(), al.data_ptr(), out.data_ptr(), width, height)
        assert_same(out.cpu().numpy(), old)
        denoise_var_device(ctx, c.data_ptr(), S.data_ptr(), nm.data_ptr(), al.data_ptr(), out.data_ptr(), var.data_ptr(),
                           width, height)
        assert_same(out.cpu().numpy(), want)
        assert_same(var.cpu().numpy(), want_var)


# ------------------------------------------------ 4. a noise session
def mean_canvas(canvases, n, sampler):
    """The CANVAS snapshot after n samples, from the oracle's one-sample canvases."""
    s, _ = NR.fold(canvases, n)
    c = np.zeros(canvases[0].shape)
    c[..., :3] = NR.mean_of(s, n, sampler)
    c[..., 3] = canvases[0][..., 3]
    return c


def host_guides(guides):
    return tuple(None if g is None else g.cpu().numpy() for g in guides)


def test_a_noise_session_denoised_equals_the_twin_of_its_snapshots(gpu):
    """cornell 40 x 30, forward accumulation, steps of 1, 2, 4, 1: from done = 3 on the filtered
    frame is the twin's over the numpy reference of the two snapshots, and the session's own
    snapshots stay the undisturbed session's (the reference's)."""
    canvases, W, H, sampler = NR.case_canvases("cornell", N.ACC_FORWARD, 8, (40, 30))
    r = GPURenderer(scene_case("cornell")[0], W, H, 8, accumulation=N.ACC_FORWARD)
    guides = r.render_guides()
    normal, albedo = host_guides(guides)
    assert normal.any() and albedo.any()
    filtered = 0
    with r.progressive(4, noise=True) as s:
        s.step(1)
        with pytest.raises(RuntimeError, match="noise: needs at least 2 samples"):
            s.denoised(guides)
        for k in (2, 4, 1):
            s.step(k)
            colour = mean_canvas(canvases, s.done, sampler)
            se = NR.reference(canvases, s.done, W, H, sampler)[0]
            got, var = s.denoised(guides)
            want, want_var = host_denoise_var(colour, se, normal, albedo)
            assert_same(got, want)
            assert_same(var, want_var)
            assert got.tobytes() != colour.tobytes() and s.denoise_ms > 0
            assert_same(s.snapshot(), colour)
            assert_same(s.snapshot(N.SNAP_NOISE), se)
            filtered += 1
        assert s.done == 8 and filtered == 3
        # other parameters, a lone guide and Gamma / Clamp reach the filter
        p = N.denoise_params(2, 3.0, 0.25, 1.0)
        got, var = s.denoised((guides[0], None), p, 1e-3, post=N.POST_GAMMA_CLAMP)
        want, want_var = host_denoise_var(colour, se, normal, None, p, 1e-3)
        live = want[..., 3] != 0
        post = want.copy()
        post[..., :3] = np.minimum(np.sqrt(want[..., :3]), 1.0)
        assert np.array_equal(got[live], post[live])
        assert_same(var, want_var)
    with r.progressive(4) as s:  # a session without the moments has no estimate to filter by
        s.step()
        with pytest.raises(RuntimeError, match="IZPI_PROG_NOISE"):
            s.denoised(guides)
    r.close()


def test_an_adaptive_session_denoised_equals_the_twin_of_its_snapshots(gpu):
    """cornell 40 x 30, forward, threshold 0.25, steps of 4 with adapt after each: the pixels
    carry several sample counts, and the snapshots (adapt_ref's) already divide by them."""
    steps = (4,) * 4
    rule = dict(threshold=0.25, floor=0.01, tolerated=0.05, min_spp=4)
    ref, W, H, sampler = AR.simulate("cornell", N.ACC_FORWARD, list(steps), rule, size=(40, 30), counters=False)
    assert len(set(ref[-1]["n"][ref[-1]["counted"]].tolist())) >= 3  # several distinct n_p
    r = GPURenderer(scene_case("cornell")[0], W, H, 16, accumulation=N.ACC_FORWARD)
    guides = r.render_guides()
    normal, albedo = host_guides(guides)
    with r.progressive(4, total=16, noise=True, adaptive=True) as s:
        for k, st in zip(steps, ref):
            s.step(k)
            got = s.adapt(**rule)
            assert got["active"] == st["adapt"]["active"]
            canvas, var = s.denoised(guides)
            want, want_var = host_denoise_var(st["canvas"], st["noise"], normal, albedo)
            assert_same(canvas, want)
            assert_same(var, want_var)
            assert_same(s.snapshot(), st["canvas"])
    r.close()


def test_a_spectral_session_is_filtered_in_xyz_before_its_post(gpu):
    import torch
    canvases, W, H, sampler = NR.case_canvases("glass_spectral", N.ACC_FORWARD, 8)
    assert sampler == N.SAMPLER_SPECTRAL
    r = GPURenderer(scene_case("glass_spectral")[0], W, H, 8, sampler=sampler, accumulation=N.ACC_FORWARD)
    guides = r.render_guides()
    assert guides[1] is None  # the Normal guide only
    normal = guides[0].cpu().numpy()
    dev = torch.device("cuda", gpu)
    with r.progressive(4, noise=True) as s:
        s.step()
        s.step()
        xyz = mean_canvas(canvases, 8, sampler)
        se = NR.reference(canvases, 8, W, H, sampler)[0]
        assert_same(s.snapshot(), xyz)
        want, want_var = host_denoise_var(xyz, se, normal, None)
        got, var = s.denoised(guides)
        assert_same(got, want)
        assert_same(var, want_var)
        got, var = s.denoised(guides, post=N.POST_SPECTRAL | N.POST_GAMMA_CLAMP)
        assert_same(var, want_var)
    a = torch.from_numpy(want).to(dev)
    b = torch.zeros_like(a)
    torch.cuda.synchronize(dev)
    r.spectral_post(a.data_ptr(), b.data_ptr())
    r.postprocess(b.data_ptr(), [(N.FILTER_GAMMA, 0.0), (N.FILTER_CLAMP, 1.0)])
    assert_same(got, b.cpu().numpy())
    with pytest.raises(ValueError):
        with r.progressive(4, noise=True, post=N.POST_SPECTRAL) as s:
            s.step()
            s.denoised(guides)
    r.close()


# ------------------------------------------------ 5. the command-line tool
def test_cli_denoise_variance_writes_the_python_path_s_frame(gpu, tmp_path):
    W, H = 40, 30
    r = GPURenderer(configs.cornell_rgb(W / H), W, H, 8, bvh="gpu", accumulation=N.ACC_FORWARD)
    guides = r.render_guides()
    with r.progressive(4, noise=True) as s:
        s.step()
        s.step()
        want, want_var = s.denoised(guides)
        p = N.denoise_params(2, 3.0, 0.25, 1.0)
        other, _ = s.denoised(guides, p, 1e-3)
    r.close()
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(W / H))
    raw, pfm, vpfm = tmp_path / "d.f64", tmp_path / "d.pfm", tmp_path / "v.pfm"
    base = [str(build.CLI), "--scene", str(box), "--x", str(W), "--y", str(H), "--samples", "8", "--progressive", "4"]
    rule = ["--noise-threshold", "0.0001"]  # (never met: the frame has all 8 samples)
    run = subprocess.run(base + rule + ["--denoise-variance", "--raw", str(raw), "--out", str(pfm), "--variance-out", str(vpfm)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stderr.splitlines() if ln.startswith("IZPI_DENOISE_VAR ")]
    assert len(lines) == 1 and lines[0].startswith("IZPI_DENOISE_VAR iterations=5 sigma_colour=%g floor=%g ms=" % (
        N.DENOISE_VAR_DEFAULT_SIGMA_COLOUR, N.DENOISE_VAR_DEFAULT_FLOOR)), run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(H, W, 4), want)
    head = b"PF\n40 30\n-1.0\n"
    for path, plane in ((pfm, want[..., :3]), (vpfm, np.repeat(want_var[..., None], 3, 2))):
        data = path.read_bytes()
        assert data.startswith(head)
        pixels = np.frombuffer(data[len(head):], "<f4").reshape(H, W, 3)[::-1]  # bottom row first
        assert np.array_equal(pixels, plane.astype(np.float32))
    # N, --denoise-sigma and --variance-floor reach the filter
    run = subprocess.run(base + rule + ["--denoise-variance", "2", "--denoise-sigma", "3,0.25,1", "--variance-floor", "0.001",
                                        "--raw", str(raw)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert_same(np.fromfile(raw, np.float64).reshape(H, W, 4), other)
    # refused without the noise estimate; --denoise with --progressive stays refused
    run = subprocess.run(base + ["--denoise-variance"], capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "--denoise-variance needs --progressive and --noise-threshold" in run.stderr
    run = subprocess.run(base + ["--denoise"], capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "not with --progressive" in run.stderr
