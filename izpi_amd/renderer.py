"""GPURenderer — the drop-in for izpi's render.Renderer (internal/render/renderer.go:26-28).

``GPURenderer(scene, W, H, spp, max_depth, ...)`` mirrors ``render.New`` (renderer.go:73-104)
and ``.render()`` mirrors ``Render(ctx) image.Image`` (renderer.go:108-222): it returns the
float64 NRGBA canvas (H, W, 4) the Go renderer fills — RGB for the Colour sampler, CIE XYZ
before post-processing for the Spectral sampler (``.render_spectral_rgb()`` applies
FireflyRejection + XYZToRGB on the GPU like renderer.go:216-219).

Multi-GPU goes through the library (include/izpi_gpu.h): the frame's tiles become the units
of izpi_host_share_units (quarter tiles, where they can be cut), the units are dealt
round-robin (unit % G == i), each device renders its units into a packed buffer, and the
shares are gathered to device 0, which scatters them into the canvas. Two forms:

* ``MultiGPURenderer`` — one process drives every GPU (izpi_gpu_multi_*): one host
  thread and stream per device, xGMI peer copies to device 0;
* ``GPURenderer.render_rank`` — one process per GPU (torchrun): the library's own RCCL
  communicator (izpi_gpu_comm_init) and one ncclGather to rank 0.

Per pixel-sample RNG streams make the image independent of the partition.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .scene import HostScene


GPU_BVH_METHOD = N.BVH_PLOC_SAH


def gpu_leaf_max(desc):
    """Primitives per leaf of the GPU-built tree for a scene (izpi_scene_desc), by the
    library's rule (izpi_host_bvh_leaf_max, shared with the Go shim): 3, or 2 when
    spheres are at least a quarter of the primitives. A sphere test (square root and two
    f64 divisions) costs more than a node visit, so sphere-heavy scenes want smaller leaves:
    C5 (10 spheres of 22 primitives) at 32 spp 876.7 -> 851.6 ms per frame with 2 (1: 931),
    C4 (2 of 16) 194.9 -> 196.8 ms, C3 (no spheres) best at 3 (profiles/r3c/c5_leaf.log)."""
    return int(N.lib().izpi_host_bvh_leaf_max(C.byref(desc)))


def _check(rc, ctx, what):
    if rc != 0:
        msg = N.lib().izpi_gpu_last_error(ctx).decode() if ctx else ""
        raise RuntimeError("%s failed (status %d): %s" % (what, rc, msg))


def build_bvh4(ctx, boxes, leaf_max=4, method=None):
    """izpi_gpu_build_bvh4 on context `ctx` over [n][6] f64 boxes: (nodes (m, 128) uint8, order, ms)."""
    if method is None:
        method = GPU_BVH_METHOD
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    n = len(boxes)
    nodes = np.zeros((max(1, 2 * n), 128), np.uint8)
    order = np.zeros(max(1, n), np.uint32)
    m = C.c_uint32()
    ms = C.c_double()
    _check(N.lib().izpi_gpu_build_bvh4(ctx, boxes.ctypes.data_as(N.c_double_p), n, leaf_max, method,
                                        nodes.ctypes.data_as(C.POINTER(N.BVH4Node)), len(nodes), C.byref(m),
                                        order.ctypes.data_as(N.c_uint32_p), C.byref(ms)),
           ctx, "izpi_gpu_build_bvh4")
    return nodes[:m.value].copy(), order[:n].copy(), ms.value


def _canvas_args(colour, normal, albedo):
    """The three input canvases as contiguous (H, W, 4) float64 arrays (guides may be None)."""
    colour = np.ascontiguousarray(colour, np.float64)
    if colour.ndim != 3 or colour.shape[2] != 4:
        raise ValueError("a canvas is (H, W, 4) float64")
    guides = []
    for g in (normal, albedo):
        if g is not None:
            g = np.ascontiguousarray(g, np.float64)
            if g.shape != colour.shape:
                raise ValueError("the guides have the colour canvas's shape")
        guides.append(g)
    return colour, guides[0], guides[1]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_denoise(colour, normal=None, albedo=None, params=None):
    """izpi_host_denoise: the denoiser's host twin over (H, W, 4) float64
    canvases; normal / albedo are the guides or None, params an N.DenoiseParams (None = the
    library's defaults). Returns the denoised canvas. Needs no GPU."""
    colour, normal, albedo = _canvas_args(colour, normal, albedo)
    out = np.zeros_like(colour)
    L = N.lib()
    rc = L.izpi_host_denoise(_ptr(colour), _ptr(normal), _ptr(albedo), _ptr(out), colour.shape[1], colour.shape[0],
                             None if params is None else C.byref(params))
    if rc != 0:
        raise RuntimeError("izpi_host_denoise failed (status %d): %s" % (rc, L.izpi_host_last_error().decode()))
    return out


def denoise(ctx, colour, normal=None, albedo=None, params=None, timing=None):
    """izpi_gpu_denoise on context `ctx` over host canvases (upload, filter, download):
    host_denoise's arguments and result, bit for bit. timing (a dict) receives "ms"."""
    colour, normal, albedo = _canvas_args(colour, normal, albedo)
    out = np.zeros_like(colour)
    ms = C.c_double()
    _check(N.lib().izpi_gpu_denoise(ctx, _ptr(colour), _ptr(normal), _ptr(albedo), _ptr(out), colour.shape[1],
                                    colour.shape[0], None if params is None else C.byref(params), C.byref(ms)),
           ctx, "izpi_gpu_denoise")
    if timing is not None:
        timing["ms"] = ms.value
    return out


def denoise_device(ctx, colour_ptr, normal_ptr, albedo_ptr, out_ptr, width, height, params=None):
    """izpi_gpu_denoise_device on context `ctx`: device pointers (normal_ptr / albedo_ptr may
    be None); returns the device ms of the iterations."""
    ms = C.c_double()
    _check(N.lib().izpi_gpu_denoise_device(ctx, C.c_void_p(colour_ptr), C.c_void_p(normal_ptr or 0),
                                           C.c_void_p(albedo_ptr or 0), C.c_void_p(out_ptr), width, height,
                                           None if params is None else C.byref(params), C.byref(ms)),
           ctx, "izpi_gpu_denoise_device")
    return ms.value


def _stderr_arg(colour, stderr):
    stderr = np.ascontiguousarray(stderr, np.float64)
    if stderr.shape != colour.shape:
        raise ValueError("the standard errors have the colour canvas's shape")
    return stderr


def _floor(variance_floor):
    return C.c_double(N.DENOISE_VAR_DEFAULT_FLOOR if variance_floor is None else float(variance_floor))


def host_denoise_var(colour, stderr, normal=None, albedo=None, params=None, variance_floor=None):
    """izpi_host_denoise_var: the variance-guided denoiser's host twin over
    (H, W, 4) float64 canvases; stderr is the canvas of standard errors (N.SNAP_NOISE's form),
    normal / albedo the guides or None, params an N.DenoiseParams (None = that filter's
    defaults), variance_floor None = N.DENOISE_VAR_DEFAULT_FLOOR. Returns (canvas, variance
    (H, W)). Needs no GPU."""
    colour, normal, albedo = _canvas_args(colour, normal, albedo)
    stderr = _stderr_arg(colour, stderr)
    out = np.zeros_like(colour)
    var = np.zeros(colour.shape[:2], np.float64)
    L = N.lib()
    rc = L.izpi_host_denoise_var(_ptr(colour), _ptr(stderr), _ptr(normal), _ptr(albedo), _ptr(out), _ptr(var),
                                 colour.shape[1], colour.shape[0], None if params is None else C.byref(params),
                                 _floor(variance_floor))
    if rc != 0:
        raise RuntimeError("izpi_host_denoise_var failed (status %d): %s" % (rc, L.izpi_host_last_error().decode()))
    return out, var


def denoise_var(ctx, colour, stderr, normal=None, albedo=None, params=None, variance_floor=None, timing=None):
    """izpi_gpu_denoise_var on context `ctx` over host canvases (upload, filter, download):
    host_denoise_var's arguments and results, bit for bit. timing (a dict) receives "ms"."""
    colour, normal, albedo = _canvas_args(colour, normal, albedo)
    stderr = _stderr_arg(colour, stderr)
    out = np.zeros_like(colour)
    var = np.zeros(colour.shape[:2], np.float64)
    ms = C.c_double()
    _check(N.lib().izpi_gpu_denoise_var(ctx, _ptr(colour), _ptr(stderr), _ptr(normal), _ptr(albedo), _ptr(out), _ptr(var),
                                        colour.shape[1], colour.shape[0], None if params is None else C.byref(params),
                                        _floor(variance_floor), C.byref(ms)),
           ctx, "izpi_gpu_denoise_var")
    if timing is not None:
        timing["ms"] = ms.value
    return out, var


def denoise_var_device(ctx, colour_ptr, stderr_ptr, normal_ptr, albedo_ptr, out_ptr, var_out_ptr, width, height,
                       params=None, variance_floor=None):
    """izpi_gpu_denoise_var_device on context `ctx`: device pointers (normal_ptr, albedo_ptr and
    var_out_ptr, the (H, W) plane, may be None); returns the device ms of the iterations."""
    ms = C.c_double()
    _check(N.lib().izpi_gpu_denoise_var_device(ctx, C.c_void_p(colour_ptr), C.c_void_p(stderr_ptr),
                                               C.c_void_p(normal_ptr or 0), C.c_void_p(albedo_ptr or 0),
                                               C.c_void_p(out_ptr), C.c_void_p(var_out_ptr or 0), width, height,
                                               None if params is None else C.byref(params), _floor(variance_floor),
                                               C.byref(ms)),
           ctx, "izpi_gpu_denoise_var_device")
    return ms.value


def host_noise(sums, moment2, done, sampler=N.SAMPLER_COLOUR, counted=None, params=None):
    """izpi_host_noise: the host twin of a progressive session's noise estimate (DESIGN.md
    3.9) over (n, 3) float64 sums and second moments after `done` samples, in packed pixel
    order; counted: a (n,) mask of the pixels the statistic counts (None: all); params an
    N.NoiseParams (None = the library's defaults). Returns (se (n, 4), stats dict). Needs no GPU."""
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 3)
    moment2 = np.ascontiguousarray(moment2, np.float64).reshape(-1, 3)
    if sums.shape != moment2.shape:
        raise ValueError("sums and moment2 are both (n, 3)")
    if counted is not None:
        counted = np.ascontiguousarray(counted, np.uint8).reshape(-1)
        if len(counted) != len(sums):
            raise ValueError("counted has one entry per pixel")
    se = np.zeros((len(sums), 4), np.float64)
    st = N.NoiseStats()
    L = N.lib()
    rc = L.izpi_host_noise(_ptr(sums), _ptr(moment2), _ptr(counted), len(sums), int(done), int(sampler),
                           None if params is None else C.byref(params), _ptr(se), C.byref(st))
    if rc != 0:
        raise RuntimeError("izpi_host_noise failed (status %d): %s" % (rc, L.izpi_host_last_error().decode()))
    return se, st.as_dict()


def host_adapt(sums, moment2, samples, active, done, sampler=N.SAMPLER_COLOUR, counted=None, params=None):
    """izpi_host_adapt: the host twin of one adapt() of an adaptive session over
    (n, 3) float64 sums and second moments in packed pixel order; samples: (n,) the pixels' own
    sample counts; active: (n,) mask of the pixels still sampled (an active pixel has `done`
    samples); counted: as host_noise's. Returns (active after the call (n,) bool, e (n,), stats
    dict); the arguments are not changed. Needs no GPU."""
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 3)
    moment2 = np.ascontiguousarray(moment2, np.float64).reshape(-1, 3)
    samples = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    active = np.array(active, np.uint8).reshape(-1)  # (a copy: the call writes it)
    if sums.shape != moment2.shape or len(samples) != len(sums) or len(active) != len(sums):
        raise ValueError("sums and moment2 are (n, 3), samples and active (n,)")
    if counted is not None:
        counted = np.ascontiguousarray(counted, np.uint8).reshape(-1)
        if len(counted) != len(sums):
            raise ValueError("counted has one entry per pixel")
    e = np.zeros(len(sums), np.float64)
    st = N.AdaptStats()
    L = N.lib()
    rc = L.izpi_host_adapt(_ptr(sums), _ptr(moment2), _ptr(counted), _ptr(samples), _ptr(active), len(sums), int(done),
                           int(sampler), None if params is None else C.byref(params), _ptr(e), C.byref(st))
    if rc != 0:
        raise RuntimeError("izpi_host_adapt failed (status %d): %s" % (rc, L.izpi_host_last_error().decode()))
    return active.astype(bool), e, st.as_dict()


def make_request(width, height, spp, max_depth, sampler, background, seed, exposure, bg_spd=None, tiles=None,
                 layout=N.OUT_CANVAS, post=N.POST_NONE, tuning=None, accumulation=N.ACC_RECURSIVE, ink=(0.0, 0.0, 0.0)):
    """izpi_render_req for Render (the arrays it points to are kept alive on `req._keep`).
    tuning: an N.RenderTuning (launch settings; None = the library's defaults).
    accumulation: N.ACC_RECURSIVE (bitwise against the oracle's recursion) or N.ACC_FORWARD.
    ink: the WireFrame sampler's edge colour (its paper is `background`)."""
    req = N.RenderReq()
    req.abi_version = N.IZPI_ABI_VERSION
    req.accumulation = accumulation
    req.ink[:] = ink
    req.post = post
    req.exposure = exposure
    req.width, req.height = width, height
    req.spp = spp
    req.max_depth = max_depth
    req.sampler = sampler
    req.out_layout = layout
    req.background[:] = background
    req.seed = seed
    keep = []
    if tiles is not None:
        t = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 4)
        keep.append(t)
        req.num_tiles = len(t)
        req.tiles = t.ctypes.data_as(C.POINTER(C.c_uint32))
    if bg_spd is not None and len(bg_spd[0]):
        wl, val = bg_spd
        keep += [wl, val]
        req.num_bg_spd = wl.size
        req.bg_spd_wavelengths = wl.ctypes.data_as(C.POINTER(C.c_double))
        req.bg_spd_values = val.ctypes.data_as(C.POINTER(C.c_double))
    if tuning is not None:
        keep.append(tuning)
        req.tuning = C.pointer(tuning)
    req._keep = keep
    return req


def common_tiles(width, height):
    """common.Tiles + grid.WalkGrid spiral order, as an (n, 4) uint32 array."""
    buf = (C.c_uint32 * (4 * (width * height // 16 + 16)))()
    n = N.lib().izpi_host_tiles(width, height, buf, len(buf) // 4)
    if n == 0:
        raise ValueError("%dx%d is not divisible by any common.Tiles step" % (width, height))
    return np.frombuffer(buf, np.uint32, count=4 * n).reshape(n, 4).copy()


class ProgressiveSession:
    """A progressive render (izpi_gpu_progressive_*, izpi_gpu_multi_progressive_*): the
    frame's samples in steps, the sums kept on the device, a snapshot after any step.
    After k samples, in any split of steps, ``snapshot()`` is the canvas ``render(spp=k)``
    returns, bit for bit, and ``stats`` holds the same counters. A context manager: leaving
    the block (or ``close()``) ends the session, which is also how a render is cancelled.

    ``done`` / ``total``: samples per pixel rendered so far, and the session's cap.
    ``stats``: cumulative since the session began (a list per device for a multi-GPU one).

    ``noise=True`` (IZPI_PROG_NOISE) also keeps the samples' second moments: ``noise()`` is
    the frame's noise statistic, ``snapshot(N.SNAP_NOISE)`` the per-pixel standard errors and
    ``converge()`` steps until the stop rule holds. The images and counters
    are those of a session without it.

    ``adaptive=True`` (with noise=True; IZPI_PROG_ADAPTIVE): ``adapt()`` retires
    the pixels whose estimate has fallen to the threshold, the steps sample the others only, and
    ``snapshot(N.SNAP_SAMPLES)`` is the map of the pixels' own sample counts. Every pixel is,
    bit for bit, that pixel of ``render(spp=its count)``. ``active``: the pixels still sampled
    (None before the first adapt()); ``done`` stops advancing once there is none."""

    def __init__(self, owner, req, step_spp, noise=False, adaptive=False):
        self._owner = owner
        self._multi = isinstance(owner, MultiGPURenderer)
        self._handle = owner.m if self._multi else owner.ctx
        self._pre = "izpi_gpu_multi_progressive_" if self._multi else "izpi_gpu_progressive_"
        self._req = req  # (the library keeps its own copy; this one sizes the snapshots)
        self.step_spp = int(step_spp)
        self.total = int(req.spp)
        self.done = 0
        self.stats = None
        self._open = False
        self.noise_stats = None
        self.adaptive = bool(adaptive)
        self.active = None
        self.adapt_stats = None
        if adaptive and not noise:
            raise ValueError("adaptive=True needs noise=True (IZPI_PROG_ADAPTIVE needs IZPI_PROG_NOISE)")
        if noise:
            self._call("begin_ex", C.byref(req), self.step_spp, N.PROG_NOISE | (N.PROG_ADAPTIVE if adaptive else 0))
        else:
            self._call("begin", C.byref(req), self.step_spp)
        self._open = True

    def _call(self, what, *args):
        rc = getattr(N.lib(), self._pre + what)(self._handle, *args)
        if self._multi:
            self._owner._check(rc, self._pre + what)
        else:
            _check(rc, self._handle, self._pre + what)

    def step(self, n=None):
        """Render the next n samples per pixel (None: step_spp), clipped to the cap; returns `done`."""
        G = len(self._owner.devices) if self._multi else 1
        st = (N.RenderStats * G)()
        self._call("step", 0 if n is None else int(n), st)
        want = self.step_spp if n is None else int(n)
        if self.active != 0:  # (an adaptive session without an active pixel renders nothing)
            self.done = min(self.total, self.done + (want if want else self.step_spp))
        self.stats = [st[i].as_dict() for i in range(G)] if self._multi else st[0].as_dict()
        self._owner.stats = self.stats
        return self.done

    def snapshot(self, form=N.SNAP_CANVAS, out=None):
        """The image after `done` samples, as a host array: N.SNAP_CANVAS is what render()
        returns at spp = done (the session's layout and post); N.SNAP_DISPLAY holds
        display.DisplayTile's pixels (B, G, R, 1.0; Spectral: ACEScg of the exposed XYZ).
        `out` (read first, like render()'s canvas) defaults to zeros."""
        if out is None:
            if self._req.out_layout == N.OUT_PACKED and not self._multi:
                out = np.zeros(N.lib().izpi_gpu_output_bytes(C.byref(self._req)) // 8, np.float64)
            else:
                out = np.zeros((self._req.height, self._req.width, 4), np.float64)
        self._call("snapshot", int(form), out.ctypes.data_as(C.c_void_p))
        return out

    @staticmethod
    def _noise_params(params, kw):
        if params is not None and kw:
            raise ValueError("give an N.NoiseParams or keyword fields, not both")
        return N.noise_params(**kw) if kw else params

    def noise(self, params=None, **kw):
        """izpi_gpu_progressive_noise: the frame's noise statistic after `done` >= 2 samples, as
        a dict (pixels, nonfinite, above, max_error, sum_error, device_ms, done, converged).
        threshold=, floor=, tolerated=, min_spp= (or an N.NoiseParams) override the defaults."""
        p = self._noise_params(params, kw)
        st = N.NoiseStats()
        self._call("noise", None if p is None else C.byref(p), C.byref(st))
        self.noise_stats = st.as_dict()
        return self.noise_stats

    def adapt(self, params=None, **kw):
        """izpi_gpu_progressive_adapt (an adaptive session after `done` >= 2 samples): retire
        every active pixel that is not counted, not finite or whose e is at most the threshold.
        Returns a dict (pixels, nonfinite, active, retired, samples, device_ms, done, converged);
        the keywords are noise()'s."""
        p = self._noise_params(params, kw)
        st = N.AdaptStats()
        self._call("adapt", None if p is None else C.byref(p), C.byref(st))
        self.adapt_stats = st.as_dict()
        self.active = self.adapt_stats["active"]
        return self.adapt_stats

    def converge(self, params=None, **kw):
        """izpi_gpu_progressive_converge: step(step_spp) and, from max(2, min_spp) samples on,
        noise(), until the frame is converged or `done` reaches the cap. Returns the last
        statistic (None when none was evaluated); `done` and `stats` are updated."""
        p = self._noise_params(params, kw)
        G = len(self._owner.devices) if self._multi else 1
        st = (N.RenderStats * G)()
        ns = N.NoiseStats()
        before = self.done
        self._call("converge", None if p is None else C.byref(p), st, C.byref(ns))
        if self.adaptive:  # (its progress counts the samples rendered; the last evaluation knows `done`)
            self.done = ns.done if ns.done else self.total
            if ns.done:
                self.active = ns.above
        else:
            d, t = self._owner.progress()  # (pixels * done, pixels * cap)
            self.done = d * self.total // t if t else self.done
        if self.done != before:
            self.stats = [st[i].as_dict() for i in range(G)] if self._multi else st[0].as_dict()
            self._owner.stats = self.stats
        self.noise_stats = ns.as_dict() if ns.done else None
        return self.noise_stats

    def snapshot_device(self, out_ptr, form=N.SNAP_CANVAS):
        """snapshot() into device memory at `out_ptr` (single-GPU sessions)."""
        if self._multi:
            raise ValueError("a multi-GPU session snapshots into host memory")
        _check(N.lib().izpi_gpu_progressive_snapshot_device(self._handle, int(form), C.c_void_p(out_ptr)), self._handle,
               "izpi_gpu_progressive_snapshot_device")

    def denoised(self, guides, params=None, variance_floor=None, post=N.POST_NONE):
        """The frame after `done` >= 2 samples through the variance-guided filter (DESIGN.md
        3.8a), of a single-GPU noise session begun with post=N.POST_NONE over the whole canvas:
        the CANVAS and the NOISE snapshot into device canvases, izpi_gpu_denoise_var_device on
        them with `guides` (GPURenderer.render_guides(), taken before the session was opened),
        then for the Spectral sampler with N.POST_SPECTRAL in `post` izpi_gpu_spectral_post of
        the filtered XYZ (the standard errors are XYZ's, so the filter runs on the sums' own
        space, ahead of FireflyRejection), then N.POST_GAMMA_CLAMP's Gamma and Clamp. An
        adaptive session needs nothing more: its snapshots already divide by the pixels' own
        counts. Returns (canvas, variance): host arrays, the variance (H, W) that of the
        filtered frame before `post`. The session's sums are not touched."""
        import torch
        if self._multi:
            raise ValueError("a multi-GPU session gathers its snapshots; filter them on izpi_gpu_multi_context(m, 0)")
        if self._req.out_layout != N.OUT_CANVAS or self._req.post != N.POST_NONE:
            raise ValueError("denoised() needs a session over the canvas begun with post=N.POST_NONE")
        r = self._owner
        spectral = self._req.sampler == N.SAMPLER_SPECTRAL
        if post & N.POST_SPECTRAL and not spectral:
            raise ValueError("N.POST_SPECTRAL needs the Spectral sampler")
        normal, albedo = guides
        dev = torch.device("cuda", r.device)
        shape = (self._req.height, self._req.width, 4)
        colour, se, out = (torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(3))
        var = torch.zeros(shape[:2], dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)  # the zero fills run on torch's stream, the library on its own
        self.snapshot_device(colour.data_ptr(), N.SNAP_CANVAS)
        self.snapshot_device(se.data_ptr(), N.SNAP_NOISE)
        self.denoise_ms = denoise_var_device(self._handle, colour.data_ptr(), se.data_ptr(),
                                             None if normal is None else normal.data_ptr(),
                                             None if albedo is None else albedo.data_ptr(), out.data_ptr(),
                                             var.data_ptr(), shape[1], shape[0], params, variance_floor)
        if post & N.POST_SPECTRAL:
            r.spectral_post(out.data_ptr(), colour.data_ptr())
            out = colour
        if post & N.POST_GAMMA_CLAMP:
            r.postprocess(out.data_ptr(), [(N.FILTER_GAMMA, 0.0), (N.FILTER_CLAMP, 1.0)])
        return out.cpu().numpy(), var.cpu().numpy()

    def close(self):
        if self._open and getattr(self._owner, "m" if self._multi else "ctx", None):
            self._open = False
            self._call("end")
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _render_adaptive(owner, threshold, step_spp, max_spp, params):
    with owner.progressive(step_spp, total=max_spp, noise=True, adaptive=True) as s:
        stats = s.converge(threshold=threshold, **params)
        return s.snapshot(), stats, s.snapshot(N.SNAP_SAMPLES)[..., 0].copy()


class GPURenderer:
    def __init__(self, scene, width, height, spp, max_depth=50, sampler=N.SAMPLER_COLOUR, background=(0.0, 0.0, 0.0),
                 spectral_background=None, device=0, seed=12345, bvh_seed=12345, host_scene=None, bvh="reference",
                 bvh_leaf_max=None, tuning=None, accumulation=N.ACC_RECURSIVE, bvh_quantized=False, ink=(0.0, 0.0, 0.0)):
        """sampler: any of render.New's five (N.SAMPLER_*, by name in izpi_amd.SAMPLERS); the
        WireFrame sampler draws edges in `ink` on a paper of `background`.
        bvh="reference": hitable.NewBVH4's tree, rebuilt bit for bit on the host (the
        parity default); bvh="gpu": the GPU linear BVH4 builder (izpi_gpu_build_bvh4),
        same node format, different topology. tuning: an
        N.RenderTuning for every request (None = library defaults). accumulation: how a
        path's radiance is summed (N.ACC_*; the attribute may be changed between frames).
        bvh_quantized: upload the tree with IZPI_SCENE_QUANTIZED_BVH (64-B nodes whose
        decoded boxes contain the exact ones: half the node memory, C3's traversal 5% slower,
        DESIGN.md 3.6); default off."""
        self.tuning = tuning
        self.bvh_quantized = bool(bvh_quantized)
        self.accumulation = int(accumulation)
        if bvh not in ("reference", "gpu"):
            raise ValueError("bvh must be 'reference' or 'gpu'")
        self.width, self.height, self.spp, self.max_depth = int(width), int(height), int(spp), int(max_depth)
        self.sampler = int(sampler)
        self.background = tuple(float(b) for b in background)
        self.ink = tuple(float(b) for b in ink)
        self.seed = int(seed)
        self.device = int(device)
        # leader mode: aspect = W/H overrides the scene camera (transport.go aspectOverride)
        self.host = host_scene or HostScene(scene, aspect_override=float(width) / float(height), bvh_seed=bvh_seed,
                                            skip_bvh=bvh == "gpu")
        if spectral_background is None:
            self._bg_wl = np.zeros(0)
            self._bg_val = np.zeros(0)
        else:
            wl, val = spectral_background
            self._bg_wl = np.ascontiguousarray(wl, np.float64)
            self._bg_val = np.ascontiguousarray(val, np.float64)
        L = N.lib()
        ctx = C.c_void_p()
        rc = L.izpi_gpu_open(self.device, C.byref(ctx))
        if rc != 0:
            raise RuntimeError("izpi_gpu_open(%d) failed: no HIP device?" % self.device)
        self.ctx = ctx
        self.bvh_build_ms = None
        self.bvh_leaf_max = (bvh_leaf_max or gpu_leaf_max(self.host.desc)) if bvh == "gpu" else None
        if bvh == "gpu" and host_scene is None:
            nodes, order, self.bvh_build_ms = self.build_bvh4(self.host.prim_boxes(),
                                                              self.bvh_leaf_max)
            self.host.set_bvh(nodes, order)
        self.host.set_flags(N.SCENE_QUANTIZED_BVH if self.bvh_quantized else 0)
        _check(L.izpi_gpu_upload_scene(ctx, C.byref(self.host.desc)), ctx, "izpi_gpu_upload_scene")
        self.stats = None

    def use_tree(self, scene, bvh, bvh_seed=12345, bvh_leaf_max=None, bvh_quantized=False):
        """Re-upload `scene` with another BVH (`bvh`, `bvh_quantized` as in __init__) into this
        context. Its render buffers stay and are reused by the next frame of the same request:
        a second renderer would allocate, and leave for the driver to clear, a second workspace."""
        self.bvh_quantized = bool(bvh_quantized)
        if bvh not in ("reference", "gpu"):
            raise ValueError("bvh must be 'reference' or 'gpu'")
        self.host = HostScene(scene, aspect_override=float(self.width) / float(self.height), bvh_seed=bvh_seed,
                              skip_bvh=bvh == "gpu")
        self.bvh_build_ms = None
        self.bvh_leaf_max = (bvh_leaf_max or gpu_leaf_max(self.host.desc)) if bvh == "gpu" else None
        if bvh == "gpu":
            nodes, order, self.bvh_build_ms = self.build_bvh4(self.host.prim_boxes(), self.bvh_leaf_max)
            self.host.set_bvh(nodes, order)
        self.host.set_flags(N.SCENE_QUANTIZED_BVH if self.bvh_quantized else 0)
        _check(N.lib().izpi_gpu_upload_scene(self.ctx, C.byref(self.host.desc)), self.ctx, "izpi_gpu_upload_scene")

    def build_bvh4(self, boxes, leaf_max=4, method=None):
        """izpi_gpu_build_bvh4 over [n][6] f64 boxes: (nodes (m, 128) uint8, order, ms)."""
        return build_bvh4(self.ctx, boxes, leaf_max, method)

    # -------------------------------------------------------------- request
    def request(self, tiles=None, layout=N.OUT_CANVAS, spp=None, post=N.POST_NONE):
        return make_request(self.width, self.height, self.spp if spp is None else int(spp), self.max_depth,
                            self.sampler, self.background, self.seed, self.exposure, (self._bg_wl, self._bg_val),
                            tiles, layout, post, self.tuning, self.accumulation, self.ink)

    # --------------------------------------------------------------- render
    @property
    def exposure(self):
        return float(self.host.desc.camera.exposure)  # Scene.Exposure = camera exposure (scene.go:30)

    def render(self, tiles=None, canvas=None, spp=None, post=N.POST_NONE):
        """Render.Render(): returns the (H, W, 4) float64 canvas (host memory). With
        post=POST_SPECTRAL (whole frame only) the XYZ canvas goes through
        FireflyRejection + XYZToRGB on the GPU, as Render does for the Spectral sampler;
        with POST_GAMMA_CLAMP the leader's png pipeline (Gamma, Clamp(1.0)) follows."""
        if canvas is None:
            canvas = np.zeros((self.height, self.width, 4), np.float64)
        req = self.request(tiles, N.OUT_CANVAS, spp, post)
        st = N.RenderStats()
        rc = N.lib().izpi_gpu_render(self.ctx, C.byref(req), canvas.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        _check(rc, self.ctx, "izpi_gpu_render")
        self.stats = st.as_dict()
        return canvas

    def prepare(self, tiles=None, layout=N.OUT_CANVAS, post=N.POST_NONE):
        """izpi_gpu_prepare: allocate the workspace of this renderer's requests ahead of the
        first frame (render.New's canvas allocation, renderer.go:73-104); after comm_init,
        this rank's share of render_rank."""
        req = self.request(tiles, layout, None, post)
        _check(N.lib().izpi_gpu_prepare(self.ctx, C.byref(req)), self.ctx, "izpi_gpu_prepare")

    def progressive(self, step_spp, total=None, tiles=None, layout=N.OUT_CANVAS, post=N.POST_NONE, noise=False,
                    adaptive=False):
        """Begin a progressive render of up to `total` samples per pixel (None: this
        renderer's spp) with a workspace sized for steps of `step_spp`: a ProgressiveSession.
        render(), prepare() and a scene upload are refused until it is closed. noise=True keeps
        the second moments the session's noise estimate needs (24 B per pixel more);
        adaptive=True (with it) lets adapt() stop the sampling of converged pixels."""
        return ProgressiveSession(self, self.request(tiles, layout, total, post), step_spp, noise, adaptive)

    def render_adaptive(self, threshold, step_spp=16, max_spp=None, **params):
        """render_until with adaptive sampling: a pixel stops taking samples once its own
        estimate is at most `threshold`. Returns (canvas, stats, samples_map): every pixel of
        the canvas is render(spp=n)'s at n = that pixel of samples_map (H, W), stats the last
        noise statistic (None when max_spp came before the first evaluation)."""
        return _render_adaptive(self, threshold, step_spp, max_spp, params)

    def render_until(self, threshold, step_spp, max_spp=None, **params):
        """Render in steps of `step_spp` until the stop rule holds at `threshold` (the other
        izpi_noise_params as keywords: floor, tolerated, min_spp) or `max_spp` samples (None:
        this renderer's spp) are spent. Returns (canvas, stats): the canvas is render()'s at
        spp = stats["done"], the samples spent; stats is the last noise statistic (None when
        max_spp came before the first evaluation: the canvas then holds max_spp samples)."""
        with self.progressive(step_spp, total=max_spp, noise=True) as s:
            stats = s.converge(threshold=threshold, **params)
            return s.snapshot(), stats

    def progress(self):
        """(samples finished, samples of the request) of the render running on this context,
        readable from another thread while render() runs (izpi_gpu_progress)."""
        d, t = C.c_uint64(), C.c_uint64()
        _check(N.lib().izpi_gpu_progress(self.ctx, C.byref(d), C.byref(t)), self.ctx, "izpi_gpu_progress")
        return d.value, t.value

    def render_spectral_rgb(self):
        """The full reference Render() for the Spectral sampler: XYZ render, then
        FireflyRejection + XYZToRGB (renderer.go:215-219), all on the GPU."""
        return self.render(post=N.POST_SPECTRAL)

    def spectral_post(self, xyz_ptr, rgba_ptr):
        """FireflyRejection + XYZToRGB of a device XYZ canvas into another device canvas."""
        _check(N.lib().izpi_gpu_spectral_post(self.ctx, C.c_void_p(xyz_ptr), C.c_void_p(rgba_ptr), self.width,
                                              self.height, C.c_double(self.exposure)), self.ctx,
               "izpi_gpu_spectral_post")

    def postprocess(self, canvas_ptr, filters):
        """postprocess.Pipeline.Apply on a device canvas, in place: filters is a list of
        (N.FILTER_GAMMA | N.FILTER_CLAMP, param) applied in order (pipeline.go:20-31)."""
        k = np.array([f[0] for f in filters], np.uint32)
        p = np.array([f[1] for f in filters], np.float64)
        _check(N.lib().izpi_gpu_postprocess(self.ctx, C.c_void_p(canvas_ptr), self.width, self.height,
                                            k.ctypes.data_as(N.c_uint32_p), p.ctypes.data_as(N.c_double_p), len(k)),
               self.ctx, "izpi_gpu_postprocess")

    def denoise_device(self, colour_ptr, normal_ptr, albedo_ptr, out_ptr, params=None):
        """izpi_gpu_denoise_device over device canvases of this renderer's size:
        normal_ptr / albedo_ptr may be None, params is an N.DenoiseParams (None = the library's
        defaults). Returns the device ms. Allowed while a progressive session is open."""
        return denoise_device(self.ctx, colour_ptr, normal_ptr, albedo_ptr, out_ptr, self.width, self.height, params)

    def render_guides(self, aov_spp=4, albedo=None):
        """The Normal frame and (albedo=True; the default for Colour, off for Spectral) the
        Albedo frame of this view at `aov_spp` samples, as device canvases (torch tensors):
        (normal, albedo or None), the guides of ProgressiveSession.denoised. Call it before the
        session is opened: renders are refused while one is open."""
        import torch
        if albedo is None:
            albedo = self.sampler != N.SAMPLER_SPECTRAL
        dev = torch.device("cuda", self.device)
        shape = (self.height, self.width, 4)
        guides = [torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(2 if albedo else 1)]
        torch.cuda.synchronize(dev)  # the zero fills run on torch's stream, the library on its own
        own, stats = self.sampler, self.stats
        try:
            for canvas, sampler in zip(guides, (N.SAMPLER_NORMAL, N.SAMPLER_ALBEDO)):
                self.sampler = sampler
                self.render_device(canvas.data_ptr(), spp=aov_spp)
        finally:
            self.sampler, self.stats = own, stats  # (the frame's, not the guides')
        return guides[0], guides[1] if albedo else None

    def render_denoised(self, spp=None, aov_spp=4, params=None, post=N.POST_NONE, albedo=None):
        """A denoised frame of this renderer's sampler (Colour, or Spectral through
        POST_SPECTRAL) at `spp` samples (None: self.spp): the frame, then the Normal frame and
        (albedo=True; the default for Colour, off for Spectral, whose scenes may carry no RGB
        albedo) the Albedo frame at `aov_spp`, all into device canvases, then the filter on
        the linear values, then `post`'s Gamma / Clamp. Returns the host canvas;
        self.last_noisy keeps the unfiltered frame (before Gamma / Clamp) and
        self.denoise_ms the filter's device time."""
        import torch
        if self.sampler not in (N.SAMPLER_COLOUR, N.SAMPLER_SPECTRAL):
            raise ValueError("render_denoised needs the Colour or the Spectral sampler")
        spectral = self.sampler == N.SAMPLER_SPECTRAL
        if albedo is None:
            albedo = not spectral
        dev = torch.device("cuda", self.device)
        shape = (self.height, self.width, 4)
        colour = torch.zeros(shape, dtype=torch.float64, device=dev)
        out = torch.zeros(shape, dtype=torch.float64, device=dev)
        guides = {name: torch.zeros(shape, dtype=torch.float64, device=dev)
                  for name in (("normal", "albedo") if albedo else ("normal",))}
        torch.cuda.synchronize(dev)  # the zero fills run on torch's stream, the library on its own
        stats = self.render_device(colour.data_ptr(), spp=spp, post=N.POST_SPECTRAL if spectral else N.POST_NONE)
        own = self.sampler
        try:
            for name, canvas in guides.items():
                self.sampler = N.SAMPLER_NORMAL if name == "normal" else N.SAMPLER_ALBEDO
                self.render_device(canvas.data_ptr(), spp=aov_spp)
        finally:
            self.sampler = own
        self.stats = stats  # the frame's, not the guides'
        self.denoise_ms = self.denoise_device(colour.data_ptr(), guides["normal"].data_ptr(),
                                              guides["albedo"].data_ptr() if albedo else None, out.data_ptr(), params)
        if post & N.POST_GAMMA_CLAMP:
            self.postprocess(out.data_ptr(), [(N.FILTER_GAMMA, 0.0), (N.FILTER_CLAMP, 1.0)])
        self.last_noisy = colour.cpu().numpy()
        return out.cpu().numpy()

    def render_device(self, out_ptr, tiles=None, layout=N.OUT_CANVAS, spp=None, post=N.POST_NONE):
        """Render into device memory at `out_ptr` (e.g. torch tensor .data_ptr())."""
        req = self.request(tiles, layout, spp, post)
        st = N.RenderStats()
        rc = N.lib().izpi_gpu_render_device(self.ctx, C.byref(req), C.c_void_p(out_ptr), C.byref(st))
        _check(rc, self.ctx, "izpi_gpu_render_device")
        self.stats = st.as_dict()
        return self.stats

    def output_doubles(self, tiles=None, layout=N.OUT_CANVAS):
        req = self.request(tiles, layout)
        return N.lib().izpi_gpu_output_bytes(C.byref(req)) // 8

    def unpack(self, tiles, packed_ptr, canvas_ptr):
        req = self.request(tiles, N.OUT_PACKED)
        _check(N.lib().izpi_gpu_unpack_tiles(self.ctx, C.byref(req), C.c_void_p(packed_ptr), C.c_void_p(canvas_ptr)),
               self.ctx, "izpi_gpu_unpack_tiles")

    # ------------------------------------------------------------ multi-GPU
    def comm_init(self, world, rank, comm_id):
        """Join the library's RCCL communicator (one process per GPU); comm_id is rank 0's
        izpi_gpu_comm_id bytes, broadcast by the launcher."""
        cid = (C.c_uint8 * N.COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        _check(N.lib().izpi_gpu_comm_init(self.ctx, world, rank, cid), self.ctx, "izpi_gpu_comm_init")

    def render_rank(self, out_ptr=None, post=N.POST_NONE, tiles=None):
        """Collective Render over the communicator: this rank's share of the frame, one
        ncclGather, and on rank 0 the assembled canvas written to device memory at
        `out_ptr` (post-processed). Returns this rank's stats."""
        req = self.request(tiles, N.OUT_CANVAS, None, post)
        st = N.RenderStats()
        rc = N.lib().izpi_gpu_render_rank(self.ctx, C.byref(req), C.c_void_p(out_ptr or 0), C.byref(st))
        _check(rc, self.ctx, "izpi_gpu_render_rank")
        self.stats = st.as_dict()
        return self.stats

    def render_distributed(self, rank, world, post=N.POST_NONE):
        """render_rank into a torch canvas on rank 0 (None elsewhere); the communicator
        must be set up (comm_init) when world > 1. Returns (canvas, stats)."""
        import torch
        dev = torch.device("cuda", self.device)
        canvas = torch.zeros((self.height, self.width, 4), dtype=torch.float64, device=dev) if rank == 0 else None
        if world == 1:
            st = self.render_device(canvas.data_ptr(), post=post)
        else:
            st = self.render_rank(canvas.data_ptr() if canvas is not None else None, post)
        return canvas, st

    def bvh_nodes(self):
        """The uploaded tree's BVH4Node records, (n, 128) uint8, with their exact boxes (a
        quantised upload tests the decoded boxes that oracle.quantize_bvh4 restates)."""
        d = self.host.desc
        nodes = np.frombuffer(bytes(C.string_at(C.addressof(d.nodes.contents), 128 * d.num_nodes)), np.uint8).reshape(-1, 128)
        return nodes.copy()

    def close(self):
        if getattr(self, "ctx", None):
            N.lib().izpi_gpu_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGPURenderer:
    """Render over several GPUs from one process (izpi_gpu_multi_*): the scene is
    replicated on every device, the frame's units (izpi_host_share_units: its tiles, cut
    into quarters where they can be) are dealt unit % G, device 0 gathers and assembles the
    canvas (sharding.py names the steps). Same arguments as GPURenderer plus ``devices``."""

    def __init__(self, scene, width, height, spp, devices, max_depth=50, sampler=N.SAMPLER_COLOUR,
                 background=(0.0, 0.0, 0.0), spectral_background=None, seed=12345, bvh_seed=12345, bvh="gpu",
                 bvh_leaf_max=None, tuning=None, accumulation=N.ACC_RECURSIVE, bvh_quantized=False, ink=(0.0, 0.0, 0.0)):
        self.tuning = tuning
        self.accumulation = int(accumulation)
        self.ink = tuple(float(b) for b in ink)
        self.bvh_quantized = bool(bvh_quantized)
        if bvh not in ("reference", "gpu"):
            raise ValueError("bvh must be 'reference' or 'gpu'")
        self.width, self.height, self.spp, self.max_depth = int(width), int(height), int(spp), int(max_depth)
        self.sampler = int(sampler)
        self.background = tuple(float(b) for b in background)
        self.seed = int(seed)
        self.devices = [int(d) for d in devices]
        if spectral_background is None:
            self._bg = (np.zeros(0), np.zeros(0))
        else:
            self._bg = tuple(np.ascontiguousarray(x, np.float64) for x in spectral_background)
        self.host = HostScene(scene, aspect_override=float(width) / float(height), bvh_seed=bvh_seed,
                              skip_bvh=bvh == "gpu")
        L = N.lib()
        m = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        rc = L.izpi_gpu_multi_open(devs, len(self.devices), C.byref(m))
        if rc != 0:
            raise RuntimeError("izpi_gpu_multi_open(%s) failed (status %d)" % (self.devices, rc))
        self.m = m
        self.bvh_build_ms = None
        self.bvh_leaf_max = (bvh_leaf_max or gpu_leaf_max(self.host.desc)) if bvh == "gpu" else None
        if bvh == "gpu":
            nodes, order, self.bvh_build_ms = build_bvh4(L.izpi_gpu_multi_context(m, 0), self.host.prim_boxes(),
                                                         self.bvh_leaf_max)
            self.host.set_bvh(nodes, order)
        self.host.set_flags(N.SCENE_QUANTIZED_BVH if self.bvh_quantized else 0)
        self._check(L.izpi_gpu_multi_upload_scene(m, C.byref(self.host.desc)), "izpi_gpu_multi_upload_scene")
        self.stats = None

    def _check(self, rc, what):
        if rc != 0:
            msg = N.lib().izpi_gpu_multi_last_error(self.m).decode()
            raise RuntimeError("%s failed (status %d): %s" % (what, rc, msg))

    @property
    def exposure(self):
        return float(self.host.desc.camera.exposure)

    def render(self, canvas=None, post=N.POST_NONE, to_host=True):
        """Render.Render over all devices. Returns the (H, W, 4) canvas (host), or None with
        to_host=False (the canvas stays on device 0: the timing form). self.stats is the
        list of per-device stats."""
        req = make_request(self.width, self.height, self.spp, self.max_depth, self.sampler, self.background,
                           self.seed, self.exposure, self._bg, None, N.OUT_CANVAS, post, self.tuning,
                           self.accumulation, self.ink)
        G = len(self.devices)
        st = (N.RenderStats * G)()
        if to_host and canvas is None:
            canvas = np.zeros((self.height, self.width, 4), np.float64)
        ptr = canvas.ctypes.data_as(C.c_void_p) if to_host else None
        self._check(N.lib().izpi_gpu_multi_render(self.m, C.byref(req), ptr, st), "izpi_gpu_multi_render")
        self.stats = [st[i].as_dict() for i in range(G)]
        return canvas if to_host else None

    def progressive(self, step_spp, total=None, tiles=None, layout=N.OUT_CANVAS, post=N.POST_NONE, noise=False,
                    adaptive=False):
        """GPURenderer.progressive over all devices: each holds a session over its share."""
        req = make_request(self.width, self.height, self.spp if total is None else int(total), self.max_depth,
                           self.sampler, self.background, self.seed, self.exposure, self._bg, tiles, layout, post,
                           self.tuning, self.accumulation, self.ink)
        return ProgressiveSession(self, req, step_spp, noise, adaptive)

    def render_adaptive(self, threshold, step_spp=16, max_spp=None, **params):
        """GPURenderer.render_adaptive over all devices: the same canvas and map."""
        return _render_adaptive(self, threshold, step_spp, max_spp, params)

    def progress(self):
        """(samples finished, samples of the request) summed over the devices (izpi_gpu_multi_progress)."""
        d, t = C.c_uint64(), C.c_uint64()
        self._check(N.lib().izpi_gpu_multi_progress(self.m, C.byref(d), C.byref(t)), "izpi_gpu_multi_progress")
        return d.value, t.value

    def prepare(self, post=N.POST_NONE):
        """izpi_gpu_multi_prepare: every device's workspace for its share, ahead of the first frame."""
        req = make_request(self.width, self.height, self.spp, self.max_depth, self.sampler, self.background,
                           self.seed, self.exposure, self._bg, None, N.OUT_CANVAS, post, self.tuning,
                           self.accumulation, self.ink)
        self._check(N.lib().izpi_gpu_multi_prepare(self.m, C.byref(req)), "izpi_gpu_multi_prepare")

    def close(self):
        if getattr(self, "m", None):
            N.lib().izpi_gpu_multi_close(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
