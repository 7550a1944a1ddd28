"""The Python front end without a device: the one request builder both renderers share
(renderer._Renderer.request over make_request), and the argument errors of the filter and
noise wrappers. A renderer is configured here without being opened: the frame parameters and
a host scene on the reference tree are all a request reads."""
import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd import renderer as R
from izpi_amd.scene import HostScene

W, H, SPP, DEPTH, SEED, EXPOSURE = 48, 32, 5, 7, 99, 0.75
BACKGROUND, INK = (0.125, 0.25, 0.5), (0.75, 0.5, 0.25)
BG_WL, BG_VAL = [400.0, 550.0, 700.0], [0.25, 0.5, 1.0]
TWO_TILES = [[0, 0, 16, 16], [16, 0, 32, 16]]
POINTERS = ("tiles", "bg_spd_wavelengths", "bg_spd_values", "tuning")
CLASSES = [R._Renderer, R.GPURenderer, R.MultiGPURenderer]

# request()'s arguments: (tiles, layout, spp, post)
CALLS = [
    (None, N.OUT_CANVAS, None, N.POST_NONE),
    (TWO_TILES, N.OUT_PACKED, 3, N.POST_NONE),
    (None, N.OUT_CANVAS, None, N.POST_SPECTRAL | N.POST_GAMMA_CLAMP),
]


@pytest.fixture(scope="module")
def host():
    scene = configs.cornell_rgb(W / H)
    scene.camera.exposure = EXPOSURE
    h = HostScene(scene, aspect_override=W / H)
    assert h.desc.camera.exposure == EXPOSURE != 1.0
    yield h
    h.close()


def new_tuning():
    return N.tuning(slots=2000, trace_chunk=3)


def configured(cls, host):
    """An instance of `cls` set up the way its __init__ sets the frame up (_Renderer.__init__,
    every parameter off its default), with no context or group opened."""
    r = cls.__new__(cls)
    R._Renderer.__init__(r, W, H, SPP, DEPTH, N.SAMPLER_SPECTRAL, BACKGROUND, (BG_WL, BG_VAL), SEED, new_tuning(),
                         N.ACC_FORWARD, INK, host=host)
    return r


def explicit(tiles, layout, spp, post, sampler=N.SAMPLER_SPECTRAL, accumulation=N.ACC_FORWARD):
    return R.make_request(W, H, SPP if spp is None else spp, DEPTH, sampler, BACKGROUND, SEED, EXPOSURE,
                          (np.array(BG_WL), np.array(BG_VAL)), tiles, layout, post, new_tuning(), accumulation, INK)


def plain_fields(req):
    out = {}
    for name, _ in N.RenderReq._fields_:
        if name not in POINTERS:
            v = getattr(req, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
    return out


def pointed_to(req):
    return {"tiles": [req.tiles[i] for i in range(4 * req.num_tiles)],
            "bg_spd_wavelengths": [req.bg_spd_wavelengths[i] for i in range(req.num_bg_spd)],
            "bg_spd_values": [req.bg_spd_values[i] for i in range(req.num_bg_spd)],
            "tuning": bytes(req.tuning.contents) if req.tuning else None}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("call", CALLS)
def test_request_is_make_request_of_the_frame_parameters(host, cls, call):
    got, want = configured(cls, host).request(*call), explicit(*call)
    assert plain_fields(got) == plain_fields(want)
    assert pointed_to(got) == pointed_to(want)
    # (the explicit request itself carries what was asked for)
    assert (got.width, got.height, got.max_depth, got.seed, got.exposure) == (W, H, DEPTH, SEED, EXPOSURE)
    assert got.spp == (SPP if call[2] is None else call[2]) and got.out_layout == call[1] and got.post == call[3]
    assert got.num_tiles == (0 if call[0] is None else 2) and got.num_bg_spd == 3
    assert list(got.background) == list(BACKGROUND) and list(got.ink) == list(INK)
    assert got.tuning.contents.slots == 2000 and got.tuning.contents.trace_chunk == 3


@pytest.mark.parametrize("cls", CLASSES)
def test_request_reads_live_attributes(host, cls):
    r = configured(cls, host)
    assert (r.request().sampler, r.request().accumulation) == (N.SAMPLER_SPECTRAL, N.ACC_FORWARD)
    r.sampler, r.accumulation = N.SAMPLER_NORMAL, N.ACC_RECURSIVE
    got, want = r.request(*CALLS[1]), explicit(*CALLS[1], sampler=N.SAMPLER_NORMAL, accumulation=N.ACC_RECURSIVE)
    assert (got.sampler, got.accumulation) == (N.SAMPLER_NORMAL, N.ACC_RECURSIVE)
    assert plain_fields(got) == plain_fields(want) and pointed_to(got) == pointed_to(want)
    r.tuning = None
    assert not r.request().tuning


@pytest.mark.parametrize("cls", CLASSES)
def test_every_request_goes_through_the_one_builder(host, cls, monkeypatch):
    built = []

    def recording(*args, **kw):
        built.append(args)
        return make_request(*args, **kw)

    make_request = R.make_request
    monkeypatch.setattr(R, "make_request", recording)
    r = configured(cls, host)
    r.request()
    r.request(TWO_TILES, N.OUT_PACKED, 3)
    assert len(built) == 2 and built[1][2] == 3
    assert cls.request is R._Renderer.request  # (neither renderer overrides it)


CANVAS = np.zeros((4, 6, 4))


@pytest.mark.parametrize("call, message", [
    (lambda: R.host_denoise(np.zeros((4, 6, 3))), r"a canvas is \(H, W, 4\) float64"),
    (lambda: R.host_denoise(np.zeros((4, 24))), r"a canvas is \(H, W, 4\) float64"),
    (lambda: R.host_denoise_var(np.zeros(96), CANVAS), r"a canvas is \(H, W, 4\) float64"),
    (lambda: R.host_denoise(CANVAS, normal=np.zeros((4, 5, 4))), "the guides have the colour canvas's shape"),
    (lambda: R.host_denoise(CANVAS, CANVAS, albedo=np.zeros((6, 4, 4))), "the guides have the colour canvas's shape"),
    (lambda: R.host_denoise_var(CANVAS, CANVAS, np.zeros((3, 6, 4))), "the guides have the colour canvas's shape"),
    (lambda: R.host_denoise_var(CANVAS, np.zeros((4, 6))), "the standard errors have the colour canvas's shape"),
    (lambda: R.host_noise(np.ones((3, 3)), np.ones((2, 3)), 4), r"sums and moment2 are both \(n, 3\)"),
    (lambda: R.host_adapt(np.ones((3, 3)), np.ones((2, 3)), np.ones(3), np.ones(3), 4), "sums and moment2 are"),
    (lambda: R.host_noise(np.ones((2, 3)), np.ones((2, 3)), 4, counted=np.ones(3)), "counted has one entry per pixel"),
    (lambda: R.host_adapt(np.ones((2, 3)), np.ones((2, 3)), np.ones(2), np.ones(2), 4, counted=np.ones(1)),
     "counted has one entry per pixel"),
])
def test_filter_and_noise_wrappers_refuse_misshapen_arrays(call, message):
    with pytest.raises(ValueError, match=message):
        call()
