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

Both renderers are a ``_Renderer``: it holds the frame parameters, builds every request
(``request``), loads the scene and its tree (``_load_scene``) and calls the library
(``_call``) by the owner's handle and entry prefix; a ``ProgressiveSession`` drives its
owner through the same ``_call``.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import checkpoint
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


def _status(rc, what, last_error):
    if rc != 0:
        raise RuntimeError("%s failed (status %d): %s" % (what, rc, last_error().decode()))


def _call(prefix, handle, name, *args):
    """The library's entry `prefix + name` on `handle` (a context with "izpi_gpu_", a group
    with "izpi_gpu_multi_"); a status other than 0 raises with the handle's last error."""
    L = N.lib()
    _status(getattr(L, prefix + name)(handle, *args), prefix + name,
            lambda: getattr(L, prefix + "last_error")(handle) if handle else b"")


def _host_call(name, *args):
    """The host entry izpi_host_`name` (no handle, no GPU), checked like _call."""
    L = N.lib()
    _status(getattr(L, "izpi_host_" + name)(*args), "izpi_host_" + name, L.izpi_host_last_error)


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
    _call("izpi_gpu_", ctx, "build_bvh4", boxes.ctypes.data_as(N.c_double_p), n, leaf_max, method,
          nodes.ctypes.data_as(C.POINTER(N.BVH4Node)), len(nodes), C.byref(m), order.ctypes.data_as(N.c_uint32_p),
          C.byref(ms))
    return nodes[:m.value].copy(), order[:n].copy(), ms.value


def _ref(struct):
    return None if struct is None else C.byref(struct)


def _ptr(a):
    """A void pointer to a host array, or from a device address (None and 0 are NULL)."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a or 0)


def _filter(ctx, name, colour, normal, albedo, out, width, height, params, var=None):
    """One call of an a-trous filter entry over host arrays or device
    addresses: izpi_gpu_`name` on context `ctx`, or with ctx None the host twin izpi_host_`name`.
    var: None for the plain filter, (stderr, var_out, variance_floor) for the variance-guided
    one. Returns the device ms of the iterations (None from a host twin)."""
    args = [colour, normal, albedo, out] if var is None else [colour, var[0], normal, albedo, out, var[1]]
    args = [_ptr(a) for a in args] + [width, height, _ref(params)]
    if var is not None:
        args.append(C.c_double(N.DENOISE_VAR_DEFAULT_FLOOR if var[2] is None else float(var[2])))
    if ctx is None:
        _host_call(name, *args)
        return None
    ms = C.c_double()
    _call("izpi_gpu_", ctx, name, *args, C.byref(ms))
    return ms.value


def _filter_arrays(ctx, name, colour, normal, albedo, params, timing=None, var=None):
    """_filter over host canvases: they are made contiguous (H, W, 4) float64 arrays (the
    guides may be None) and the results allocated. var: None, or (stderr, variance_floor).
    Returns the filtered canvas, with `var` (canvas, variance (H, W)); timing receives "ms"."""
    colour = np.ascontiguousarray(colour, np.float64)
    if colour.ndim != 3 or colour.shape[2] != 4:
        raise ValueError("a canvas is (H, W, 4) float64")
    guides = [g if g is None else np.ascontiguousarray(g, np.float64) for g in (normal, albedo)]
    if any(g is not None and g.shape != colour.shape for g in guides):
        raise ValueError("the guides have the colour canvas's shape")
    out = np.zeros_like(colour)
    if var is not None:
        stderr = np.ascontiguousarray(var[0], np.float64)
        if stderr.shape != colour.shape:
            raise ValueError("the standard errors have the colour canvas's shape")
        var = (stderr, np.zeros(colour.shape[:2], np.float64), var[1])
    ms = _filter(ctx, name, colour, guides[0], guides[1], out, colour.shape[1], colour.shape[0], params, var)
    if timing is not None:
        timing["ms"] = ms
    return out if var is None else (out, var[1])


def host_denoise(colour, normal=None, albedo=None, params=None):
    """izpi_host_denoise: the denoiser's host twin over (H, W, 4) float64
    canvases; normal / albedo are the guides or None, params an N.DenoiseParams (None = the
    library's defaults). Returns the denoised canvas. Needs no GPU."""
    return _filter_arrays(None, "denoise", colour, normal, albedo, params)


def denoise(ctx, colour, normal=None, albedo=None, params=None, timing=None):
    """izpi_gpu_denoise on context `ctx` over host canvases (upload, filter, download):
    host_denoise's arguments and result, bit for bit. timing (a dict) receives "ms"."""
    return _filter_arrays(ctx, "denoise", colour, normal, albedo, params, timing)


def denoise_device(ctx, colour_ptr, normal_ptr, albedo_ptr, out_ptr, width, height, params=None):
    """izpi_gpu_denoise_device on context `ctx`: device pointers (normal_ptr / albedo_ptr may
    be None); returns the device ms of the iterations."""
    return _filter(ctx, "denoise_device", colour_ptr, normal_ptr, albedo_ptr, out_ptr, width, height, params)


def host_denoise_var(colour, stderr, normal=None, albedo=None, params=None, variance_floor=None):
    """izpi_host_denoise_var: the variance-guided denoiser's host twin over
    (H, W, 4) float64 canvases; stderr is the canvas of standard errors (N.SNAP_NOISE's form),
    normal / albedo the guides or None, params an N.DenoiseParams (None = that filter's
    defaults), variance_floor None = N.DENOISE_VAR_DEFAULT_FLOOR. Returns (canvas, variance
    (H, W)). Needs no GPU."""
    return _filter_arrays(None, "denoise_var", colour, normal, albedo, params, None, (stderr, variance_floor))


def denoise_var(ctx, colour, stderr, normal=None, albedo=None, params=None, variance_floor=None, timing=None):
    """izpi_gpu_denoise_var on context `ctx` over host canvases (upload, filter, download):
    host_denoise_var's arguments and results, bit for bit. timing (a dict) receives "ms"."""
    return _filter_arrays(ctx, "denoise_var", colour, normal, albedo, params, timing, (stderr, variance_floor))


def denoise_var_device(ctx, colour_ptr, stderr_ptr, normal_ptr, albedo_ptr, out_ptr, var_out_ptr, width, height,
                       params=None, variance_floor=None):
    """izpi_gpu_denoise_var_device on context `ctx`: device pointers (normal_ptr, albedo_ptr and
    var_out_ptr, the (H, W) plane, may be None); returns the device ms of the iterations."""
    return _filter(ctx, "denoise_var_device", colour_ptr, normal_ptr, albedo_ptr, out_ptr, width, height, params,
                   (stderr_ptr, var_out_ptr, variance_floor))


def _pixel_arrays(sums, moment2, counted, per_pixel=(), shapes="sums and moment2 are both (n, 3)"):
    """host_noise's and host_adapt's arrays in packed pixel order: (n, 3) float64 sums and second
    moments and the (n,) uint8 mask `counted` (None: all), checked against each other and against
    the (n,) arrays `per_pixel`; `shapes` is what a mismatch of those says."""
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 3)
    moment2 = np.ascontiguousarray(moment2, np.float64).reshape(-1, 3)
    if sums.shape != moment2.shape or any(len(a) != len(sums) for a in per_pixel):
        raise ValueError(shapes)
    if counted is not None:
        counted = np.ascontiguousarray(counted, np.uint8).reshape(-1)
        if len(counted) != len(sums):
            raise ValueError("counted has one entry per pixel")
    return sums, moment2, counted


def host_noise(sums, moment2, done, sampler=N.SAMPLER_COLOUR, counted=None, params=None):
    """izpi_host_noise: the host twin of a progressive session's noise estimate (DESIGN.md
    3.9) over (n, 3) float64 sums and second moments after `done` samples, in packed pixel
    order; counted: a (n,) mask of the pixels the statistic counts (None: all); params an
    N.NoiseParams (None = the library's defaults). Returns (se (n, 4), stats dict). Needs no GPU."""
    sums, moment2, counted = _pixel_arrays(sums, moment2, counted)
    se = np.zeros((len(sums), 4), np.float64)
    st = N.NoiseStats()
    _host_call("noise", _ptr(sums), _ptr(moment2), _ptr(counted), len(sums), int(done), int(sampler), _ref(params),
               _ptr(se), C.byref(st))
    return se, st.as_dict()


def host_adapt(sums, moment2, samples, active, done, sampler=N.SAMPLER_COLOUR, counted=None, params=None):
    """izpi_host_adapt: the host twin of one adapt() of an adaptive session over
    (n, 3) float64 sums and second moments in packed pixel order; samples: (n,) the pixels' own
    sample counts; active: (n,) mask of the pixels still sampled (an active pixel has `done`
    samples); counted: as host_noise's. Returns (active after the call (n,) bool, e (n,), stats
    dict); the arguments are not changed. Needs no GPU."""
    samples = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    active = np.array(active, np.uint8).reshape(-1)  # (a copy: the call writes it)
    sums, moment2, counted = _pixel_arrays(sums, moment2, counted, (samples, active),
                                           "sums and moment2 are (n, 3), samples and active (n,)")
    e = np.zeros(len(sums), np.float64)
    st = N.AdaptStats()
    _host_call("adapt", _ptr(sums), _ptr(moment2), _ptr(counted), _ptr(samples), _ptr(active), len(sums), int(done),
               int(sampler), _ref(params), _ptr(e), C.byref(st))
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

    def __init__(self, owner, req, step_spp, noise=False, adaptive=False, resume=None):
        self._open = False
        if adaptive and not noise:
            raise ValueError("adaptive=True needs noise=True (IZPI_PROG_ADAPTIVE needs IZPI_PROG_NOISE)")
        if resume is not None:
            return self._resume(owner, req, step_spp, resume)
        self._owner = owner
        self._req = req  # (the library keeps its own copy; this one sizes the snapshots)
        self.step_spp = int(step_spp)
        self.total = int(req.spp)
        self.done = 0
        self.stats = None
        self.noise_stats = None
        self.adaptive = bool(adaptive)
        self.active = None
        self.adapt_stats = None
        if noise:
            self._call("begin_ex", C.byref(req), self.step_spp, N.PROG_NOISE | (N.PROG_ADAPTIVE if adaptive else 0))
        else:
            self._call("begin", C.byref(req), self.step_spp)
        self._open = True

    def _resume(self, owner, req, step_spp, resume):
        """The session a checkpoint (bytes or a path) holds, continued under `req` (DESIGN.md
        3.11): whether it keeps a noise estimate and is adaptive is the checkpoint's to say."""
        blob = checkpoint.load(resume)
        info = checkpoint.checkpoint_info(blob)
        self._owner = owner
        self._req = req
        self.step_spp = int(step_spp)
        self.total = int(req.spp)
        self.stats = self.noise_stats = self.adapt_stats = None
        self._call("resume", C.byref(req), self.step_spp, owner.scene_tag, blob, len(blob))
        self._open = True
        self.done = info["done"]
        self.adaptive = info["adaptive"]
        self.active = info["active"] if self.adaptive else None

    def _call(self, what, *args):
        self._owner._call("progressive_" + what, *args)

    def checkpoint(self):
        """izpi_gpu_progressive_checkpoint: the session's state as one self-describing blob of
        bytes, which ``progressive(..., resume=blob)`` of this or another
        renderer of the same scene and frame continues, bit for bit the uninterrupted session,
        in another process or over another number of GPUs. Legal after the first step; the
        session goes on as it was."""
        n = C.c_uint64()
        self._call("checkpoint_bytes", C.byref(n))
        buf = C.create_string_buffer(n.value)
        self._call("checkpoint", self._owner.scene_tag, buf, n.value)
        return buf.raw

    def save(self, path):
        """checkpoint() into the file `path`, through a temporary file and a rename."""
        checkpoint.save(self.checkpoint(), path)

    def step(self, n=None):
        """Render the next n samples per pixel (None: step_spp), clipped to the cap; returns `done`."""
        st = self._owner._stats_out()
        self._call("step", 0 if n is None else int(n), st)
        want = self.step_spp if n is None else int(n)
        if self.active != 0:  # (an adaptive session without an active pixel renders nothing)
            self.done = min(self.total, self.done + (want if want else self.step_spp))
        self.stats = self._owner._keep_stats(st)
        return self.done

    def snapshot(self, form=N.SNAP_CANVAS, out=None):
        """The image after `done` samples, as a host array: N.SNAP_CANVAS is what render()
        returns at spp = done (the session's layout and post); N.SNAP_DISPLAY holds
        display.DisplayTile's pixels (B, G, R, 1.0; Spectral: ACEScg of the exposed XYZ).
        `out` (read first, like render()'s canvas) defaults to zeros."""
        if out is None:
            if self._req.out_layout == N.OUT_PACKED and not self._owner._group:  # (a group assembles the canvas)
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
        st = N.NoiseStats()
        self._call("noise", _ref(self._noise_params(params, kw)), C.byref(st))
        self.noise_stats = st.as_dict()
        return self.noise_stats

    def adapt(self, params=None, **kw):
        """izpi_gpu_progressive_adapt (an adaptive session after `done` >= 2 samples): retire
        every active pixel that is not counted, not finite or whose e is at most the threshold.
        Returns a dict (pixels, nonfinite, active, retired, samples, device_ms, done, converged);
        the keywords are noise()'s."""
        st = N.AdaptStats()
        self._call("adapt", _ref(self._noise_params(params, kw)), C.byref(st))
        self.adapt_stats = st.as_dict()
        self.active = self.adapt_stats["active"]
        return self.adapt_stats

    def converge(self, params=None, **kw):
        """izpi_gpu_progressive_converge: step(step_spp) and, from max(2, min_spp) samples on,
        noise(), until the frame is converged or `done` reaches the cap. Returns the last
        statistic (None when none was evaluated); `done` and `stats` are updated."""
        st = self._owner._stats_out()
        ns = N.NoiseStats()
        before = self.done
        self._call("converge", _ref(self._noise_params(params, kw)), st, C.byref(ns))
        if self.adaptive:  # (its progress counts the samples rendered; the last evaluation knows `done`)
            self.done = ns.done if ns.done else self.total
            if ns.done:
                self.active = ns.above
        else:
            d, t = self._owner.progress()  # (pixels * done, pixels * cap)
            self.done = d * self.total // t if t else self.done
        if self.done != before:
            self.stats = self._owner._keep_stats(st)
        self.noise_stats = ns.as_dict() if ns.done else None
        return self.noise_stats

    def snapshot_device(self, out_ptr, form=N.SNAP_CANVAS):
        """snapshot() into device memory at `out_ptr` (single-GPU sessions)."""
        if self._owner._group:
            raise ValueError("a multi-GPU session snapshots into host memory")
        self._call("snapshot_device", int(form), C.c_void_p(out_ptr))

    def denoised(self, guides, params=None, variance_floor=None, post=N.POST_NONE, demodulate=False):
        """The frame after `done` >= 2 samples through the variance-guided filter (DESIGN.md
        3.8a), of a single-GPU noise session begun with post=N.POST_NONE over the whole canvas:
        the CANVAS and the NOISE snapshot into device canvases, izpi_gpu_denoise_var_device on
        them with `guides` (GPURenderer.render_guides(), taken before the session was opened),
        then for the Spectral sampler with N.POST_SPECTRAL in `post` izpi_gpu_spectral_post of
        the filtered XYZ (the standard errors are XYZ's, so the filter runs on the sums' own
        space, ahead of FireflyRejection), then N.POST_GAMMA_CLAMP's Gamma and Clamp. An
        adaptive session needs nothing more: its snapshots already divide by the pixels' own
        counts. Returns (canvas, variance): host arrays, the variance (H, W) that of the
        filtered frame before `post`. The session's sums are not touched.
        demodulate=True sets N.DENOISE_DEMODULATE on `params` (or on the defaults): the filter
        runs on colour / albedo and the albedo is multiplied back; `guides`
        must hold the Albedo frame, and the variance returned is the demodulated canvas's. The
        dividing albedo wants at least the frame's samples: take the guides with
        render_guides(aov_spp=the session's cap). A 4-sample albedo under a 64-sample frame
        measured worse than no filter (the last row of 3.8b's table)."""
        r = self._owner
        if r._group:
            raise ValueError("a multi-GPU session gathers its snapshots; filter them on izpi_gpu_multi_context(m, 0)")
        if self._req.out_layout != N.OUT_CANVAS or self._req.post != N.POST_NONE:
            raise ValueError("denoised() needs a session over the canvas begun with post=N.POST_NONE")
        if post & N.POST_SPECTRAL and self._req.sampler != N.SAMPLER_SPECTRAL:
            raise ValueError("N.POST_SPECTRAL needs the Spectral sampler")
        normal, albedo = guides
        if demodulate:
            if albedo is None:
                raise ValueError("demodulate=True needs guides with the Albedo frame")
            params = N.denoise_var_params(demodulate=True) if params is None else N.DenoiseParams.from_buffer_copy(params)
            params.flags |= N.DENOISE_DEMODULATE
        shape = (self._req.height, self._req.width, 4)
        colour, se, out, var = r._device_zeros(shape, shape, shape, shape[:2])
        self.snapshot_device(colour.data_ptr(), N.SNAP_CANVAS)
        self.snapshot_device(se.data_ptr(), N.SNAP_NOISE)
        self.denoise_ms = denoise_var_device(r.ctx, colour.data_ptr(), se.data_ptr(),
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
        if self._open and self._owner._handle:  # (a closed owner has ended its session)
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


class _Renderer:
    """What GPURenderer and MultiGPURenderer share: the frame parameters and the one request
    built from them, the scene and tree loader, and the call path into the library. A subclass
    names its entries' prefix and the attribute that holds its handle, and opens that handle.
    `sampler`, `accumulation` and `tuning` may be changed between frames: every request reads
    them anew. Building a request needs no device: the parameters and `host` are enough."""

    _prefix = None  # "izpi_gpu_" or "izpi_gpu_multi_": <prefix><name> are the entries, <prefix>last_error the error
    _handle_attr = None  # the attribute that holds the library's handle (None once closed)
    _group = False  # a group of devices: stats are a list per device, snapshots come to the host

    def __init__(self, width, height, spp, max_depth=50, sampler=N.SAMPLER_COLOUR, background=(0.0, 0.0, 0.0),
                 spectral_background=None, seed=12345, tuning=None, accumulation=N.ACC_RECURSIVE, ink=(0.0, 0.0, 0.0),
                 host=None):
        self.tuning = tuning
        self.accumulation = int(accumulation)
        self.width, self.height, self.spp, self.max_depth = int(width), int(height), int(spp), int(max_depth)
        self.sampler = int(sampler)
        self.background = tuple(float(b) for b in background)
        self.ink = tuple(float(b) for b in ink)
        self.seed = int(seed)
        wl, val = (np.zeros(0), np.zeros(0)) if spectral_background is None else spectral_background
        self._bg_spd = (np.ascontiguousarray(wl, np.float64), np.ascontiguousarray(val, np.float64))
        self.host = host
        self.stats = None

    # ------------------------------------------------------------- the library
    @property
    def _handle(self):
        return getattr(self, self._handle_attr, None) if self._handle_attr else None

    def _call(self, name, *args):
        _call(self._prefix, self._handle, name, *args)

    def _stats_out(self):
        """The izpi_render_stats a render entry fills: one, or one per device of a group."""
        return (N.RenderStats * (len(self.devices) if self._group else 1))()

    def _keep_stats(self, st):
        self.stats = [s.as_dict() for s in st] if self._group else st[0].as_dict()
        return self.stats

    def _load_scene(self, scene, bvh, bvh_seed, bvh_leaf_max, bvh_quantized, tree_ctx, host_scene=None):
        """Build `scene`'s HostScene with the tree `bvh` names ("reference": hitable.NewBVH4's,
        rebuilt on the host; "gpu": izpi_gpu_build_bvh4 on the context `tree_ctx`) and upload it
        through this renderer's upload_scene entry. A given `host_scene` is uploaded as it is."""
        if bvh not in ("reference", "gpu"):
            raise ValueError("bvh must be 'reference' or 'gpu'")
        self.bvh_quantized = bool(bvh_quantized)
        # leader mode: aspect = W/H overrides the scene camera (transport.go aspectOverride)
        self.host = host_scene or HostScene(scene, aspect_override=float(self.width) / float(self.height),
                                            bvh_seed=bvh_seed, skip_bvh=bvh == "gpu")
        self.bvh_build_ms = None
        self.bvh_leaf_max = (bvh_leaf_max or gpu_leaf_max(self.host.desc)) if bvh == "gpu" else None
        if bvh == "gpu" and host_scene is None:
            nodes, order, self.bvh_build_ms = build_bvh4(tree_ctx, self.host.prim_boxes(), self.bvh_leaf_max)
            self.host.set_bvh(nodes, order)
        self.host.set_flags(N.SCENE_QUANTIZED_BVH if self.bvh_quantized else 0)
        self._call("upload_scene", C.byref(self.host.desc))

    # -------------------------------------------------------------- request
    @property
    def exposure(self):
        return float(self.host.desc.camera.exposure)  # Scene.Exposure = camera exposure (scene.go:30)

    def request(self, tiles=None, layout=N.OUT_CANVAS, spp=None, post=N.POST_NONE):
        return make_request(self.width, self.height, self.spp if spp is None else int(spp), self.max_depth,
                            self.sampler, self.background, self.seed, self.exposure, self._bg_spd,
                            tiles, layout, post, self.tuning, self.accumulation, self.ink)

    # ------------------------------------------------------------- sessions
    @property
    def scene_tag(self):
        """izpi_host_scene_tag of the host scene this renderer uploaded: what its sessions'
        checkpoints carry and a resume compares. Computed on first use."""
        if getattr(self, "_scene_tag_of", None) is not self.host:
            self._scene_tag, self._scene_tag_of = checkpoint.scene_tag(self.host.desc), self.host
        return self._scene_tag

    def progressive(self, step_spp, total=None, tiles=None, layout=N.OUT_CANVAS, post=N.POST_NONE, noise=False,
                    adaptive=False, resume=None):
        """Begin a progressive render of up to `total` samples per pixel (None: this
        renderer's spp) with a workspace sized for steps of `step_spp`: a ProgressiveSession
        (of a group: each device holds a session over its share). render(), prepare() and a
        scene upload are refused until it is closed. noise=True keeps the second moments the
        session's noise estimate needs (24 B per pixel more); adaptive=True (with it) lets
        adapt() stop the sampling of converged pixels. resume: a checkpoint (the bytes of
        ProgressiveSession.checkpoint(), or the path save() wrote) to continue instead of
        starting at zero: noise and adaptive are then the checkpoint's; total (at least the
        samples done), step_spp, layout, post and the tiles' order and shape may be new."""
        return ProgressiveSession(self, self.request(tiles, layout, total, post), step_spp, noise, adaptive, resume)

    def render_adaptive(self, threshold, step_spp=16, max_spp=None, **params):
        """render_until with adaptive sampling: a pixel stops taking samples once its own
        estimate is at most `threshold`. Returns (canvas, stats, samples_map): every pixel of
        the canvas is render(spp=n)'s at n = that pixel of samples_map (H, W), stats the last
        noise statistic (None when max_spp came before the first evaluation). A group returns
        the same canvas and map."""
        with self.progressive(step_spp, total=max_spp, noise=True, adaptive=True) as s:
            stats = s.converge(threshold=threshold, **params)
            return s.snapshot(), stats, s.snapshot(N.SNAP_SAMPLES)[..., 0].copy()

    def progress(self):
        """(samples finished, samples of the request) of the render running on this context
        (summed over a group's devices), readable from another thread while render() runs
        (izpi_gpu_progress, izpi_gpu_multi_progress)."""
        d, t = C.c_uint64(), C.c_uint64()
        self._call("progress", C.byref(d), C.byref(t))
        return d.value, t.value

    def close(self):
        if self._handle:
            getattr(N.lib(), self._prefix + "close")(self._handle)
            setattr(self, self._handle_attr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GPURenderer(_Renderer):
    _prefix = "izpi_gpu_"
    _handle_attr = "ctx"

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
        super().__init__(width, height, spp, max_depth, sampler, background, spectral_background, seed, tuning,
                         accumulation, ink)
        self.device = int(device)
        ctx = C.c_void_p()
        if N.lib().izpi_gpu_open(self.device, C.byref(ctx)) != 0:
            raise RuntimeError("izpi_gpu_open(%d) failed: no HIP device?" % self.device)
        self.ctx = ctx
        self._load_scene(scene, bvh, bvh_seed, bvh_leaf_max, bvh_quantized, ctx, host_scene)

    def use_tree(self, scene, bvh, bvh_seed=12345, bvh_leaf_max=None, bvh_quantized=False):
        """Re-upload `scene` with another BVH (`bvh`, `bvh_quantized` as in __init__) into this
        context. Its render buffers stay and are reused by the next frame of the same request:
        a second renderer would allocate, and leave for the driver to clear, a second workspace."""
        self._load_scene(scene, bvh, bvh_seed, bvh_leaf_max, bvh_quantized, self.ctx)

    def build_bvh4(self, boxes, leaf_max=4, method=None):
        """izpi_gpu_build_bvh4 over [n][6] f64 boxes: (nodes (m, 128) uint8, order, ms)."""
        return build_bvh4(self.ctx, boxes, leaf_max, method)

    # --------------------------------------------------------------- render
    def _render(self, name, req, out):
        st = self._stats_out()
        self._call(name, C.byref(req), out, st)
        return self._keep_stats(st)

    def render(self, tiles=None, canvas=None, spp=None, post=N.POST_NONE):
        """Render.Render(): returns the (H, W, 4) float64 canvas (host memory). With
        post=POST_SPECTRAL (whole frame only) the XYZ canvas goes through
        FireflyRejection + XYZToRGB on the GPU, as Render does for the Spectral sampler;
        with POST_GAMMA_CLAMP the leader's png pipeline (Gamma, Clamp(1.0)) follows."""
        if canvas is None:
            canvas = np.zeros((self.height, self.width, 4), np.float64)
        self._render("render", self.request(tiles, N.OUT_CANVAS, spp, post), canvas.ctypes.data_as(N.c_double_p))
        return canvas

    def prepare(self, tiles=None, layout=N.OUT_CANVAS, post=N.POST_NONE):
        """izpi_gpu_prepare: allocate the workspace of this renderer's requests ahead of the
        first frame (render.New's canvas allocation, renderer.go:73-104); after comm_init,
        this rank's share of render_rank."""
        self._call("prepare", C.byref(self.request(tiles, layout, None, post)))

    def render_until(self, threshold, step_spp, max_spp=None, **params):
        """Render in steps of `step_spp` until the stop rule holds at `threshold` (the other
        izpi_noise_params as keywords: floor, tolerated, min_spp) or `max_spp` samples (None:
        this renderer's spp) are spent. Returns (canvas, stats): the canvas is render()'s at
        spp = stats["done"], the samples spent; stats is the last noise statistic (None when
        max_spp came before the first evaluation: the canvas then holds max_spp samples)."""
        with self.progressive(step_spp, total=max_spp, noise=True) as s:
            stats = s.converge(threshold=threshold, **params)
            return s.snapshot(), stats

    def render_spectral_rgb(self):
        """The full reference Render() for the Spectral sampler: XYZ render, then
        FireflyRejection + XYZToRGB (renderer.go:215-219), all on the GPU."""
        return self.render(post=N.POST_SPECTRAL)

    def spectral_post(self, xyz_ptr, rgba_ptr):
        """FireflyRejection + XYZToRGB of a device XYZ canvas into another device canvas."""
        self._call("spectral_post", C.c_void_p(xyz_ptr), C.c_void_p(rgba_ptr), self.width, self.height,
                   C.c_double(self.exposure))

    def postprocess(self, canvas_ptr, filters):
        """postprocess.Pipeline.Apply on a device canvas, in place: filters is a list of
        (N.FILTER_GAMMA | N.FILTER_CLAMP, param) applied in order (pipeline.go:20-31)."""
        k = np.array([f[0] for f in filters], np.uint32)
        p = np.array([f[1] for f in filters], np.float64)
        self._call("postprocess", C.c_void_p(canvas_ptr), self.width, self.height, k.ctypes.data_as(N.c_uint32_p),
                   p.ctypes.data_as(N.c_double_p), len(k))

    def denoise_device(self, colour_ptr, normal_ptr, albedo_ptr, out_ptr, params=None):
        """izpi_gpu_denoise_device over device canvases of this renderer's size:
        normal_ptr / albedo_ptr may be None, params is an N.DenoiseParams (None = the library's
        defaults). Returns the device ms. Allowed while a progressive session is open."""
        return denoise_device(self.ctx, colour_ptr, normal_ptr, albedo_ptr, out_ptr, self.width, self.height, params)

    def _device_zeros(self, *shapes):
        """Zeroed float64 device arrays (torch tensors) of `shapes` that the library may write."""
        import torch
        dev = torch.device("cuda", self.device)
        arrays = [torch.zeros(shape, dtype=torch.float64, device=dev) for shape in shapes]
        torch.cuda.synchronize(dev)  # the zero fills run on torch's stream, the library on its own
        return arrays

    def render_guides(self, aov_spp=4, albedo=None):
        """The Normal frame and (albedo=True; the default for Colour, off for Spectral) the
        Albedo frame of this view at `aov_spp` samples, as device canvases (torch tensors):
        (normal, albedo or None), the guides of ProgressiveSession.denoised. Call it before the
        session is opened: renders are refused while one is open. Guides for
        denoised(demodulate=True) want `aov_spp` at the session's cap: the albedo a frame is
        divided by must come from at least the frame's samples (a 4-sample albedo under a
        64-sample frame measured worse than no filter, the last row of DESIGN.md 3.8b's table)."""
        if albedo is None:
            albedo = self.sampler != N.SAMPLER_SPECTRAL
        guides = self._device_zeros(*[(self.height, self.width, 4)] * (2 if albedo else 1))
        own, stats = self.sampler, self.stats
        try:
            for canvas, sampler in zip(guides, (N.SAMPLER_NORMAL, N.SAMPLER_ALBEDO)):
                self.sampler = sampler
                self.render_device(canvas.data_ptr(), spp=aov_spp)
        finally:
            self.sampler, self.stats = own, stats  # (the frame's, not the guides')
        return guides[0], guides[1] if albedo else None

    def render_denoised(self, spp=None, aov_spp=None, params=None, post=N.POST_NONE, albedo=None, demodulate=False):
        """A denoised frame of this renderer's sampler (Colour, or Spectral through
        POST_SPECTRAL) at `spp` samples (None: self.spp): the frame, then the Normal frame and
        (albedo=True; the default for Colour, off for Spectral, whose scenes may carry no RGB
        albedo) the Albedo frame at `aov_spp`, all into device canvases, then the filter on
        the linear values, then `post`'s Gamma / Clamp. Returns the host canvas;
        self.last_noisy keeps the unfiltered frame (before Gamma / Clamp) and
        self.denoise_ms the filter's device time. aov_spp None means 4, or with demodulate
        the frame's `spp`. demodulate=True (Colour only) sets N.DENOISE_DEMODULATE on `params`
        (or on the defaults): the filter runs on colour / albedo and the albedo is multiplied
        back, which keeps texture detail."""
        if self.sampler not in (N.SAMPLER_COLOUR, N.SAMPLER_SPECTRAL):
            raise ValueError("render_denoised needs the Colour or the Spectral sampler")
        spectral = self.sampler == N.SAMPLER_SPECTRAL
        if demodulate:
            if spectral:
                raise ValueError("demodulate=True needs the Colour sampler: a Spectral frame has no Albedo guide")
            if albedo is not None and not albedo:
                raise ValueError("demodulate=True needs the Albedo frame: not with albedo=False")
            params = N.denoise_params(demodulate=True) if params is None else N.DenoiseParams.from_buffer_copy(params)
            params.flags |= N.DENOISE_DEMODULATE
        if aov_spp is None:
            aov_spp = (self.spp if spp is None else spp) if demodulate else 4
        colour, out = self._device_zeros(*[(self.height, self.width, 4)] * 2)
        self.render_device(colour.data_ptr(), spp=spp, post=N.POST_SPECTRAL if spectral else N.POST_NONE)
        normal, albedo = self.render_guides(aov_spp, not spectral if albedo is None else albedo)
        self.denoise_ms = self.denoise_device(colour.data_ptr(), normal.data_ptr(),
                                              None if albedo is None else albedo.data_ptr(), out.data_ptr(), params)
        if post & N.POST_GAMMA_CLAMP:
            self.postprocess(out.data_ptr(), [(N.FILTER_GAMMA, 0.0), (N.FILTER_CLAMP, 1.0)])
        self.last_noisy = colour.cpu().numpy()
        return out.cpu().numpy()

    def render_device(self, out_ptr, tiles=None, layout=N.OUT_CANVAS, spp=None, post=N.POST_NONE):
        """Render into device memory at `out_ptr` (e.g. torch tensor .data_ptr())."""
        return self._render("render_device", self.request(tiles, layout, spp, post), C.c_void_p(out_ptr))

    def output_doubles(self, tiles=None, layout=N.OUT_CANVAS):
        req = self.request(tiles, layout)
        return N.lib().izpi_gpu_output_bytes(C.byref(req)) // 8

    def unpack(self, tiles, packed_ptr, canvas_ptr):
        self._call("unpack_tiles", C.byref(self.request(tiles, N.OUT_PACKED)), C.c_void_p(packed_ptr),
                   C.c_void_p(canvas_ptr))

    # ------------------------------------------------------------ multi-GPU
    def comm_init(self, world, rank, comm_id):
        """Join the library's RCCL communicator (one process per GPU); comm_id is rank 0's
        izpi_gpu_comm_id bytes, broadcast by the launcher."""
        self._call("comm_init", world, rank, (C.c_uint8 * N.COMM_ID_BYTES).from_buffer_copy(bytes(comm_id)))

    def render_rank(self, out_ptr=None, post=N.POST_NONE, tiles=None):
        """Collective Render over the communicator: this rank's share of the frame, one
        ncclGather, and on rank 0 the assembled canvas written to device memory at
        `out_ptr` (post-processed). Returns this rank's stats."""
        return self._render("render_rank", self.request(tiles, N.OUT_CANVAS, None, post), C.c_void_p(out_ptr or 0))

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


class MultiGPURenderer(_Renderer):
    """Render over several GPUs from one process (izpi_gpu_multi_*): the scene is
    replicated on every device, the frame's units (izpi_host_share_units: its tiles, cut
    into quarters where they can be) are dealt unit % G, device 0 gathers and assembles the
    canvas (sharding.py names the steps). Same arguments as GPURenderer plus ``devices``."""

    _prefix = "izpi_gpu_multi_"
    _handle_attr = "m"
    _group = True

    def __init__(self, scene, width, height, spp, devices, max_depth=50, sampler=N.SAMPLER_COLOUR,
                 background=(0.0, 0.0, 0.0), spectral_background=None, seed=12345, bvh_seed=12345, bvh="gpu",
                 bvh_leaf_max=None, tuning=None, accumulation=N.ACC_RECURSIVE, bvh_quantized=False, ink=(0.0, 0.0, 0.0)):
        super().__init__(width, height, spp, max_depth, sampler, background, spectral_background, seed, tuning,
                         accumulation, ink)
        self.devices = [int(d) for d in devices]
        m = C.c_void_p()
        rc = N.lib().izpi_gpu_multi_open((C.c_int * len(self.devices))(*self.devices), len(self.devices), C.byref(m))
        if rc != 0:
            raise RuntimeError("izpi_gpu_multi_open(%s) failed (status %d)" % (self.devices, rc))
        self.m = m
        self._load_scene(scene, bvh, bvh_seed, bvh_leaf_max, bvh_quantized, N.lib().izpi_gpu_multi_context(m, 0))

    def render(self, canvas=None, post=N.POST_NONE, to_host=True):
        """Render.Render over all devices. Returns the (H, W, 4) canvas (host), or None with
        to_host=False (the canvas stays on device 0: the timing form). self.stats is the
        list of per-device stats."""
        if to_host and canvas is None:
            canvas = np.zeros((self.height, self.width, 4), np.float64)
        st = self._stats_out()
        ptr = canvas.ctypes.data_as(C.c_void_p) if to_host else None
        self._call("render", C.byref(self.request(post=post)), ptr, st)
        self._keep_stats(st)
        return canvas if to_host else None

    def prepare(self, post=N.POST_NONE):
        """izpi_gpu_multi_prepare: every device's workspace for its share, ahead of the first frame."""
        self._call("prepare", C.byref(self.request(post=post)))
