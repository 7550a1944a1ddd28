"""Albedo demodulation of the two a-trous denoisers without a GPU: the
host twins (izpi_host_denoise, izpi_host_denoise_var with IZPI_DENOISE_DEMODULATE) against the
Python restatement (tests/denoise_demod_ref.py) to the byte, canvas and variance plane; hand
cases that follow from the rule; the argument checks; a stand-alone program under
AddressSanitizer and UBSan; and the measurement the option exists for: on a textured box both
demodulated filters beat their plain selves and the unfiltered frame."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import host_denoise, host_denoise_var
from izpi_amd.scene import Scene
from oracle import oracle as O
from tests import denoise_demod_ref as MR
from tests import noise_ref as NR
from tests import preview_ref as PR

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"
FLOOR = 2.0 ** -10


def same(got, want):
    return got.tobytes() == want.tobytes()


# ------------------------------------------------------------ 1. twin == restatement
@pytest.mark.parametrize("case", MR.cases(), ids=MR.case_id)
def test_fixed_filter_twin_equals_the_restatement_bytewise(case):
    w, h, n, guides = case
    c, _, nm, al = MR.seeded(w, h)
    keep_c, keep_a = c.copy(), al.copy()
    nm, al = MR.pick_guides(nm, al, guides)
    got = host_denoise(c, nm, al, N.denoise_params(iterations=n, demodulate=True))
    want = MR.reference(case, False)
    assert same(got, want), "canvas: max |diff| %g" % np.nanmax(np.abs(got - want))
    assert same(c, keep_c) and same(al, keep_a)  # the inputs are read only
    plain = host_denoise(c, nm, al, N.denoise_params(iterations=n))
    if n == 0:
        assert same(got, c) and same(got, plain)  # a copy, flag or not
    elif w * h > 1:
        assert not same(got, c) and not same(got, plain)  # it did something, and something else
    if h > 1:
        assert same(got[0], c[0])  # the dead row
    if w >= 8 and h >= 8:
        cy, cx = h // 2, w // 3
        assert same(got[cy, cx], c[cy, cx])  # the NaN pixel
        assert same(got[3, 2], c[3, 2])  # 1e308 / 2^-10 overflows: the input comes back
        mask = np.ones((h, w), bool)
        mask[cy, cx] = False
        assert np.isfinite(got[mask]).all()  # neither reached a neighbour


@pytest.mark.parametrize("case", MR.cases(), ids=MR.case_id)
def test_variance_filter_twin_equals_the_restatement_bytewise(case):
    w, h, n, guides = case
    c, S, nm, al = MR.seeded(w, h)
    keep_c, keep_s, keep_a = c.copy(), S.copy(), al.copy()
    nm, al = MR.pick_guides(nm, al, guides)
    got, var = host_denoise_var(c, S, nm, al, N.denoise_var_params(iterations=n, demodulate=True))
    want, want_var = MR.reference(case, True)
    assert same(got, want), "canvas: max |diff| %g" % np.nanmax(np.abs(got - want))
    assert same(var, want_var), "variance: max |diff| %g" % np.nanmax(np.abs(var - want_var))
    assert same(c, keep_c) and same(S, keep_s) and same(al, keep_a)
    plain, plain_var = host_denoise_var(c, S, nm, al, N.denoise_var_params(iterations=n))
    if n == 0:
        assert same(got, c) and same(got, plain) and same(var, plain_var)  # a copy and the colour's V_0
    elif w * h > 1:
        assert not same(got, c) and not same(got, plain) and not same(var, plain_var)
    if h > 1:
        assert same(got[0], c[0])
    if w >= 8 and h >= 8:
        cy, cx = h // 2, w // 3
        for y, x in ((cy, cx), (3, 2), (cy - 2, cx + 1)):  # NaN colour, overflowed quotient, NaN standard error
            assert same(got[y, x], c[y, x]), (y, x)
        mask = np.ones((h, w), bool)
        mask[cy, cx] = False
        assert np.isfinite(got[mask]).all()


# ------------------------------------------------------------ 2. hand cases
def _texture(size=24, seed=5):
    """An albedo of contrast 0.2 between neighbours (a checkerboard over a seeded base), the
    colour it gives under one constant irradiance, and standard errors in proportion."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    al = np.ones((size, size, 4))
    al[..., :3] = rng.uniform(0.3, 0.6, 3) + 0.2 * ((xx + yy) % 2)[..., None] + rng.uniform(0.0, 0.02, (size, size, 3))
    L = 0.75
    c = np.ones((size, size, 4))
    c[..., :3] = al[..., :3] * L
    S = np.ones((size, size, 4))
    S[..., :3] = al[..., :3] * 0.05
    return c, S, al


SIGMAS = [(1.0, 0.5, 0.5), (4.0, 0.5, float("inf")), (0.05, 0.5, 0.01), (float("inf"), float("inf"), float("inf"))]


@pytest.mark.parametrize("sigmas", SIGMAS, ids=lambda s: "c%g-a%g" % (s[0], s[2]))
def test_a_texture_under_constant_light_is_preserved(sigmas):
    """C = A * L: D_0 = C / A is L to an ulp, the filter averages values within an ulp of each
    other, and the product with A is C again to a few ulps, whatever the sigmas weigh."""
    c, S, al = _texture()
    fixed = host_denoise(c, None, al, N.denoise_params(5, *sigmas, demodulate=True))
    guided, _ = host_denoise_var(c, S, None, al, N.denoise_params(5, *sigmas, demodulate=True))
    for got in (fixed, guided):
        rel = np.abs(got[..., :3] - c[..., :3]) / c[..., :3]
        assert rel.max() <= 1e-12, rel.max()
        assert same(got[..., 3], c[..., 3])


def test_without_the_flag_the_same_texture_is_smeared():
    """The same calls at the defaults without the flag: the texel contrast of 0.2 is below
    sigma_albedo's reach, and some pixel moves by far more than 1e-3 (measured: 0.063 for the fixed filter, 0.008 for the variance-guided one)."""
    c, S, al = _texture()
    fixed = host_denoise(c, None, al)
    guided, _ = host_denoise_var(c, S, None, al)
    for got in (fixed, guided):
        moved = np.abs(got[..., :3] - c[..., :3]).max()
        print("moved %.4f" % moved)
        assert moved > 1e-3


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "variance"])
def test_a_channel_at_the_floor_round_trips_exactly(var):
    """Channel 1's albedo is at or below the floor, negative, NaN or +Inf everywhere, the other
    channels' is 1: the flagged call is the unflagged one over a canvas (and standard errors)
    scaled by 2^10 in channel 1, scaled back. Both scalings are exact, so bit for bit."""
    c, S, nm, _ = MR.seeded(40, 30)
    c[3, 2, 0] = 0.5  # (no overflow here: the whole frame is live but row 0 and the NaN pixel)
    al = np.ones_like(c)
    specials = np.array([0.0, 2.0 ** -12, FLOOR, -0.3, 2.0 ** -11])
    yy, xx = np.mgrid[0:30, 0:40]
    al[..., 1] = specials[(3 * yy + xx) % len(specials)]
    al[11, 7, 1] = float("nan")
    al[20, 30, 1] = float("inf")
    scaled_c, scaled_s = c.copy(), S.copy()
    scaled_c[..., 1] *= 1024.0
    scaled_s[..., 1] *= 1024.0
    if var:
        got, gvar = host_denoise_var(c, S, nm, al, N.denoise_var_params(demodulate=True))
        want, wvar = host_denoise_var(scaled_c, scaled_s, nm, al)
        assert same(gvar, wvar)
    else:
        got = host_denoise(c, nm, al, N.denoise_params(demodulate=True))
        want = host_denoise(scaled_c, nm, al)
    want = want.copy()
    want[..., 1] /= 1024.0
    assert same(got, want), np.nanmax(np.abs(got - want))
    assert not same(got, c)


def test_a_pixel_not_live_in_iteration_0_is_the_input_bit_for_bit():
    c, S, al = _texture(12)
    c[2, 2] = (0.3, 0.4, 0.5, 0.0)  # never written
    c[4, 4, 0] = float("nan")
    c[6, 6, 2] = float("-inf")
    c[8, 8, 1] = 1e308  # ... over a floor albedo: the quotient is +Inf
    al[8, 8, 1] = 0.0
    dead = [(2, 2), (4, 4), (6, 6), (8, 8)]
    fixed = host_denoise(c, None, al, N.denoise_params(demodulate=True))
    S[3, 7, 1] = float("nan")  # V_0 NaN
    S[7, 3, 0] = 1e200  # V_0 +Inf
    guided, gvar = host_denoise_var(c, S, None, al, N.denoise_var_params(demodulate=True))
    for y, x in dead:
        assert same(fixed[y, x], c[y, x]) and same(guided[y, x], c[y, x]), (y, x)
    for y, x in ((3, 7), (7, 3)):
        assert same(guided[y, x], c[y, x]), (y, x)
    assert np.isnan(gvar[3, 7]) and np.isposinf(gvar[7, 3])  # their V_0 is handed through
    live = np.ones((12, 12), bool)
    for y, x in dead:
        live[y, x] = False
    assert np.isfinite(fixed[live]).all()


# ------------------------------------------------------------ 3. argument checks
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(var, flags, albedo=True, params=True):
    L = N.lib()
    c = np.ones((4, 4, 4))
    S = np.full((4, 4, 4), 0.1)
    al = np.full((4, 4, 4), 0.5) if albedo else None
    out = np.full((4, 4, 4), 7.0)
    p = (N.denoise_var_params() if var else N.denoise_params()) if params else None
    if p is not None:
        p.flags = flags
    ref = None if p is None else C.byref(p)
    if var:
        rc = L.izpi_host_denoise_var(_p(c), _p(S), None, _p(al), _p(out), None, 4, 4, ref, N.DENOISE_VAR_DEFAULT_FLOOR)
    else:
        rc = L.izpi_host_denoise(_p(c), None, _p(al), _p(out), 4, 4, ref)
    return rc, L.izpi_host_last_error().decode(), out


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "variance"])
@pytest.mark.parametrize("flags", [1, 2, 3, 5, 8, 0x80000004])
def test_every_other_flag_word_is_refused_with_the_unchanged_message(var, flags):
    rc, msg, out = _call(var, flags)
    assert rc == N.IZPI_ERR_INVALID and msg == "denoise: flags must be 0", (rc, msg)
    assert (out == 7.0).all()


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "variance"])
def test_the_flag_needs_the_albedo_canvas(var):
    rc, msg, out = _call(var, N.DENOISE_DEMODULATE, albedo=False)
    assert rc == N.IZPI_ERR_INVALID and msg == "denoise: demodulation needs the albedo canvas", (rc, msg)
    assert (out == 7.0).all()
    rc, _, out = _call(var, N.DENOISE_DEMODULATE)
    assert rc == N.IZPI_OK and np.allclose(out, 1.0, rtol=1e-14, atol=0)  # a constant frame stays, to a few ulps
    rc, _, _ = _call(var, 0, albedo=False)
    assert rc == N.IZPI_OK


def test_the_flag_is_declared_for_every_entry():
    """The six entries take one izpi_denoise_params: the flag and the floor are the header's,
    the ctypes mirror's and the params builders'; the device entries are declared, not run."""
    gpu_h = (ROOT / "include" / "izpi_gpu.h").read_text()
    assert int(re.search(r"^#define IZPI_DENOISE_DEMODULATE (\d+)u?\b", gpu_h, re.M).group(1)) == N.DENOISE_DEMODULATE == 4
    assert float(re.search(r"^#define IZPI_DENOISE_ALBEDO_FLOOR (\S+)", gpu_h, re.M).group(1)) == N.DENOISE_ALBEDO_FLOOR == FLOOR
    assert N.denoise_params(demodulate=True).flags == 4 and N.denoise_var_params(demodulate=True).flags == 4
    assert N.denoise_params().flags == 0 and N.denoise_var_params().flags == 0
    L = N.lib()
    for name in ("izpi_gpu_denoise_device", "izpi_gpu_denoise", "izpi_host_denoise", "izpi_gpu_denoise_var_device",
                 "izpi_gpu_denoise_var", "izpi_host_denoise_var"):
        assert name in N.EXPORTS and hasattr(L, name)
    assert "IZPI_DENOISE_DEMODULATE" in (ROOT / "INTEGRATION.md").read_text()
    assert N.IZPI_ABI_VERSION == 4 and L.izpi_abi_struct_size(len(N.ABI_STRUCTS)) == 0  # no new struct
    assert C.sizeof(N.DenoiseParams) == 32


def test_null_params_mean_no_demodulation():
    c, S, nm, al = MR.seeded(37, 19)
    assert same(host_denoise(c, nm, al), host_denoise(c, nm, al, N.denoise_params()))
    assert not same(host_denoise(c, nm, al), host_denoise(c, nm, al, N.denoise_params(demodulate=True)))
    a = host_denoise_var(c, S, nm, al)
    b = host_denoise_var(c, S, nm, al, N.denoise_var_params())
    d = host_denoise_var(c, S, nm, al, N.denoise_var_params(demodulate=True))
    assert same(a[0], b[0]) and same(a[1], b[1]) and not same(a[0], d[0]) and not same(a[1], d[1])
    assert _call(False, 0, params=False)[0] == N.IZPI_OK and _call(True, 0, albedo=False, params=False)[0] == N.IZPI_OK


# ------------------------------------------------------------ sanitizer program
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "denoise_demod_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "denoise_demod_check.cpp"),
                    str(CSRC / "denoise_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {ln.split()[1] for ln in lines if ln.startswith("case ")}
    assert ran >= {"40x30", "1x1", "1x7", "37x19", "hand", "arguments"}, ran


# ------------------------------------------------------------ 4. it keeps the texture and filters the light
def textured_lambert_box():
    """tests/test_gpu_parity_materials.py's scene of that name (that module is a GPU one):
    Lambert walls and a sphere with an image albedo, next to constant ones."""
    s = Scene("textured_lambert")
    alb, _, _, _ = configs._pbr_textures(s, res=32)
    mats = configs.rgb_box_materials(s)
    mats["White"] = s.lambert(albedo=alb)
    for v0, v1, v2, mname, _ in configs._BOX:
        P = np.array([v0, v1, v2], np.float64)
        span = P.max(0) - P.min(0)
        ax = [i for i in range(3) if span[i] > 0][:2]
        uv = [(P[k, ax[0]] / 100.0, P[k, ax[1]] / 100.0) for k in range(3)]
        s.add_triangles([v0], [v1], [v2], mats[mname], uv=[[c for p in uv for c in p]])
    s.add_sphere((35, 20, 45), 18, s.lambert(albedo=alb))
    configs.cornell_camera(s, 1.0)
    return s


PAIRS = [(4, 4), (16, 16), (64, 64), (64, 4)]  # the frame's samples, the guides' samples


@functools.lru_cache(maxsize=None)
def textured_measurement():
    """textured_lambert_box() at 48 x 48, seed 12345, forward accumulation: 64 one-sample
    canvases from the oracle (tests/noise_ref.py), the truth the oracle at 4096 spp with seed
    777, Normal / Albedo guides from the preview reference (the first n of one set of 64 samples
    per pixel: the frame's own primary rays), section 3.8's mask. Per (frame, guides) pair the
    RMSE of: the frame, izpi_host_denoise, the same demodulated, izpi_host_denoise_var, the same
    demodulated; all at their defaults."""
    W = H = 48
    scene = textured_lambert_box()
    canvases = NR.sample_canvases(scene, W, H, 64, N.SAMPLER_COLOUR, N.ACC_FORWARD, seed=12345)
    o = O.OracleScene(scene, aspect_override=W / H)
    req = N.RenderReq(width=W, height=H, spp=4096, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=777,
                      abi_version=N.IZPI_ABI_VERSION, accumulation=N.ACC_FORWARD)
    truth = o.render(req, threads=16)[0].reshape(H, W, 4)
    o.close()
    ref = PR.PreviewRef(scene, W, H, 64)
    samples = {N.SAMPLER_NORMAL: ref.normal_samples(), N.SAMPLER_ALBEDO: ref.albedo_samples()}
    guides = {}
    for n in (4, 16, 64):
        ref.spp = n  # (canvas() folds `spp` samples per pixel: here the first n of the 64)
        guides[n] = [ref.canvas([s for k in range(0, len(all_s), 64) for s in all_s[k:k + n]]).reshape(H, W, 4)
                     for all_s in (samples[N.SAMPLER_NORMAL], samples[N.SAMPLER_ALBEDO])]
    ref.close()
    mask = (truth[..., 3] != 0) & (truth[..., :3] <= 1.0).all(axis=2)

    def rmse(img):
        return float(np.sqrt(((img[..., :3] - truth[..., :3])[mask] ** 2).mean()))

    def frame(n):
        s, m2 = NR.fold(canvases, n)
        se, _, _ = NR.pixel_rule(s, m2, n, N.SAMPLER_COLOUR, N.NOISE_DEFAULT_FLOOR)
        c = np.zeros((H, W, 4))
        c[..., :3] = NR.mean_of(s, n, N.SAMPLER_COLOUR)
        c[..., 3] = canvases[0][..., 3]
        S = np.zeros((H, W, 4))
        S[..., :3] = se
        S[..., 3] = c[..., 3]
        S[c[..., 3] == 0] = 0.0
        return c, S

    out = {}
    for n, g in PAIRS:
        c, S = frame(n)
        nm, al = guides[g]
        out[(n, g)] = (rmse(c), rmse(host_denoise(c, nm, al)),
                       rmse(host_denoise(c, nm, al, N.denoise_params(demodulate=True))),
                       rmse(host_denoise_var(c, S, nm, al)[0]),
                       rmse(host_denoise_var(c, S, nm, al, N.denoise_var_params(demodulate=True))[0]))
    return out, int(mask.sum())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dspp-guides%d" % p)
def test_demodulation_beats_the_plain_filters_on_a_textured_scene(pair):
    """Measured through the host twins at the defaults (RMSE over the 2207 masked pixels:
    unfiltered / section 3.8 / 3.8 demodulated / section 3.8a / 3.8a demodulated), the figures
    of DESIGN.md section 3.8b:
      4 spp / guides 4 spp     0.1005 / 0.0654 / 0.0570 / 0.0629 / 0.0596
      16 spp / guides 16 spp   0.0538 / 0.0588 / 0.0392 / 0.0417 / 0.0389
      64 spp / guides 64 spp   0.0291 / 0.0567 / 0.0339 / 0.0249 / 0.0233
      64 spp / guides 4 spp    0.0291 / 0.0565 / 0.0384 / 0.0264 / 0.0326
    The last pair (a 4-sample albedo under a 64-sample frame) is printed, not asserted: it
    documents that the dividing albedo wants at least the frame's samples."""
    rows, pixels = textured_measurement()
    noisy, fixed, fixed_d, guided, guided_d = rows[pair]
    print("%d spp / guides %d spp (%d pixels): unfiltered %.4f, 3.8 %.4f, 3.8 demodulated %.4f, 3.8a %.4f, "
          "3.8a demodulated %.4f" % (pair + (pixels, noisy, fixed, fixed_d, guided, guided_d)))
    if pair in ((4, 4), (16, 16)):
        assert fixed_d < fixed
        assert fixed_d < noisy
    if pair in ((16, 16), (64, 64)):
        assert guided_d < guided
        assert guided_d < noisy
