"""The variance-guided a-trous denoiser without a GPU: the host twin
(izpi_host_denoise_var, izpi_amd/csrc/denoise_host.cpp) against the Python restatement
(tests/denoise_var_ref.py) to the byte, canvas and variance plane; hand cases that follow from
the rule; the argument checks; the entries' declarations; a stand-alone program under
AddressSanitizer and UBSan; and the measurement the filter exists for: on a Cornell box it
beats both the unfiltered frame and the filter of section 3.8 where that one makes a
well-sampled frame worse."""
import ctypes as C
import functools
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import host_denoise, host_denoise_var
from oracle import oracle as O
from tests import denoise_ref as DR
from tests import denoise_var_ref as VR
from tests import noise_ref as NR
from tests import preview_ref as PR

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"
NEW = ("izpi_gpu_denoise_var_device", "izpi_gpu_denoise_var", "izpi_host_denoise_var")


def same(got, want):
    return got.tobytes() == want.tobytes()


# ------------------------------------------------------------ 1. twin == restatement
@pytest.mark.parametrize("case", VR.cases(), ids=VR.case_id)
def test_twin_equals_the_restatement_bytewise(case):
    w, h, variant, n, guides = case
    c, S, nm, al = VR.seeded(w, h, variant=variant)
    keep_c, keep_s = c.copy(), S.copy()
    nm, al = DR.pick_guides(nm, al, guides)
    got, var = host_denoise_var(c, S, nm, al, N.denoise_var_params(iterations=n))
    want, want_var = VR.reference(case)
    assert same(got, want), "canvas: max |diff| %g" % np.nanmax(np.abs(got - want))
    assert same(var, want_var), "variance: max |diff| %g" % np.nanmax(np.abs(var - want_var))
    assert same(c, keep_c) and same(S, keep_s)  # the inputs are read only
    v0 = np.array(VR.variance0(S.tolist()))
    if n == 0:
        assert same(got, c) and same(var, v0)  # a copy, and V_0
    elif w * h > 1:
        assert not same(got, c) and not same(var, v0)  # it did something
    if variant == "dead_row0":
        assert same(got[0], c[0]) and same(var[0], v0[0])
    cy, cx = h // 2, w // 3
    if variant in ("nan_pixel", "inf_pixel", "nan_stderr", "inf_stderr"):
        assert same(got[cy, cx], c[cy, cx]) and same(var[cy, cx], v0[cy, cx])  # copied through, its V too
        mask = np.ones((h, w), bool)
        mask[cy, cx] = False
        assert np.isfinite(got[mask]).all() and np.isfinite(var[mask]).all()  # and it reached no neighbour
    if variant == "nan_guide":
        assert np.isfinite(got).all() and np.isfinite(var).all()
    if variant == "zero_stderr" and n:
        assert (var[cy:cy + 5, cx:cx + 6] > 0).all()  # the neighbours' variance came in with their colour


def test_null_params_are_the_defaults():
    c, S, nm, al = VR.seeded(37, 19)
    a = host_denoise_var(c, S, nm, al)
    b = host_denoise_var(c, S, nm, al, N.denoise_params(5, N.DENOISE_VAR_DEFAULT_SIGMA_COLOUR, 0.5, 0.5),
                         N.DENOISE_VAR_DEFAULT_FLOOR)
    assert same(a[0], b[0]) and same(a[1], b[1])
    p = N.denoise_var_params()
    assert (p.iterations, p.flags, p.sigma_colour, p.sigma_normal, p.sigma_albedo) == (5, 0, N.DENOISE_VAR_DEFAULT_SIGMA_COLOUR, 0.5, 0.5)
    text = (ROOT / "include" / "izpi_gpu.h").read_text()
    for name in ("FLOOR", "SIGMA_COLOUR"):  # the header's constants are the ctypes mirror's
        value = re.search(r"^#define IZPI_DENOISE_VAR_DEFAULT_%s (\S+)" % name, text, re.M).group(1)
        assert float(value) == getattr(N, "DENOISE_VAR_DEFAULT_" + name)
    other = host_denoise_var(c, S, nm, al, variance_floor=10 * N.DENOISE_VAR_DEFAULT_FLOOR)
    assert not same(other[0], a[0])  # the floor reaches the filter


# ------------------------------------------------------------ 2. hand cases
def _flat(colour=0.5, se=0.1, size=9):
    c = np.ones((size, size, 4))
    c[..., :3] = colour
    S = np.ones((size, size, 4))
    S[..., :3] = se
    return c, S


def test_a_constant_frame_keeps_its_colour_and_its_variance_falls_by_the_b3_gain():
    """Every e is 0, so w = h * h: the colour is an average of equal values, and V_1 =
    V_0 * sum((h_i h_j)^2) / 1^2 = V_0 * (sum h^2)^2 = V_0 * (35/128)^2 at a pixel whose 25
    taps are all inside the frame."""
    c, S = _flat()
    got, var = host_denoise_var(c, S, params=N.denoise_var_params(iterations=1))
    assert same(got, c)
    v0 = (0.1 * 0.1 + 0.1 * 0.1) + 0.1 * 0.1
    want = v0 * (35.0 / 128.0) ** 2
    assert abs(var[4, 4] - want) <= 1e-12 * want, (var[4, 4], want)
    assert var[0, 0] > var[4, 4]  # fewer taps in a corner


def test_a_pixel_without_variance_still_averages_with_equal_neighbours():
    """V = 0 does not freeze a pixel: e = dc * kc = 0 * kc = 0 whatever kc is, so its taps weigh
    h * h as everyone's, and it takes its neighbours' variance: all 25 terms but its own."""
    c, S = _flat()
    S[4, 4, :3] = 0.0
    got, var = host_denoise_var(c, S, params=N.denoise_var_params(iterations=1))
    assert same(got, c)
    v0 = (0.1 * 0.1 + 0.1 * 0.1) + 0.1 * 0.1
    want = v0 * ((35.0 / 128.0) ** 2 - (9.0 / 64.0) ** 2)
    assert abs(var[4, 4] - want) <= 1e-12 * want, (var[4, 4], want)


def test_a_pixel_without_variance_stays_put_among_other_colours():
    """All variances 0: kc = 1 / (s2 * floor). A centre 0.05 off its neighbours in every channel
    has dc = 0.0075; each other tap weighs at most h * exp(-dc * kc), their h sum to 55/64
    against the centre's 9/64, so the centre moves by at most (55/9) * 0.05 * exp(-dc * kc),
    which is below exp(-dc / (s2 * floor)) itself (about 7e-9 here)."""
    c, S = _flat(se=0.0)
    c[4, 4, :3] = 0.55
    s2, floor = 4.0, 1e-4
    got, var = host_denoise_var(c, S, params=N.denoise_var_params(iterations=1, sigma_colour=2.0), variance_floor=floor)
    bound = math.exp(-(3 * 0.05 * 0.05) / (s2 * floor))
    moved = np.abs(got[4, 4, :3] - 0.55).max()
    print("moved %.3g, bound %.3g" % (moved, bound))
    assert 1e-12 < bound < 1e-8 and moved <= bound
    assert (var == 0).all()
    # with the variance of a real estimate the same centre is pulled in
    S[..., :3] = 0.1
    got, _ = host_denoise_var(c, S, params=N.denoise_var_params(iterations=1, sigma_colour=2.0), variance_floor=floor)
    assert got[4, 4, 0] < 0.54


def test_a_normal_edge_stops_the_filter_exactly():
    """tests/test_denoise.py's edge case: exp(-2e6) is 0, so a pixel only ever sums its own
    side, where every tap has the centre's colour; sigma_colour = +Inf makes kc = 1 / Inf = 0."""
    c = np.ones((24, 24, 4))
    c[:, 12:, :3] = 0.0
    nm = np.zeros((24, 24, 4))
    nm[:, :12, 0] = 1.0
    nm[:, 12:, 1] = 1.0
    S = np.ones((24, 24, 4))
    S[..., :3] = 0.2
    got, var = host_denoise_var(c, S, nm, None, N.denoise_params(5, sigma_colour=float("inf"), sigma_normal=1e-3))
    assert same(got, c)
    assert (var > 0).all() and (var < 0.12).all()


# ------------------------------------------------------------ 3. argument checks
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(colour, S, out, var, w, h, params, floor=N.DENOISE_VAR_DEFAULT_FLOOR, normal=None):
    L = N.lib()
    rc = L.izpi_host_denoise_var(_p(colour), _p(S), _p(normal), None, _p(out), _p(var), w, h,
                                 None if params is None else C.byref(params), floor)
    return rc, L.izpi_host_last_error().decode()


MESSAGES = {
    "alias": "denoise: out may not overlap an input canvas",
    "out_is_stderr": "denoise: out may not overlap an input canvas",
    "out_is_variance": "denoise: out may not overlap the variance output",
    "variance_is_stderr": "denoise: the variance output may not overlap an input canvas",
    "variance_is_normal": "denoise: the variance output may not overlap an input canvas",
    "no_stderr": "denoise: the standard errors must be given",
    "no_colour": "denoise: colour and out must be given",
    "nine_iterations": "denoise: at most 8 iterations",
    "sigma_zero": "denoise: every sigma must be greater than 0 (+Inf drops its term)",
    "sigma_nan": "denoise: every sigma must be greater than 0 (+Inf drops its term)",
    "sigma_negative": "denoise: every sigma must be greater than 0 (+Inf drops its term)",
    "zero_width": "denoise: width and height must be at least 1",
    "zero_height": "denoise: width and height must be at least 1",
    "flags": "denoise: flags must be 0",
    "floor_zero": "denoise: variance_floor must be finite and greater than 0",
    "floor_negative": "denoise: variance_floor must be finite and greater than 0",
    "floor_nan": "denoise: variance_floor must be finite and greater than 0",
    "floor_inf": "denoise: variance_floor must be finite and greater than 0",
}


@pytest.mark.parametrize("what", sorted(MESSAGES))
def test_bad_arguments_are_refused_with_a_message(what):
    c = np.ones((4, 4, 4))
    S = np.full((4, 4, 4), 0.1)
    nm = np.ones((4, 4, 4))
    out = np.full((4, 4, 4), 7.0)
    var = np.full((4, 4), 7.0)
    p = N.denoise_var_params()
    w = h = 4
    floor = N.DENOISE_VAR_DEFAULT_FLOOR
    writes = True
    if what == "alias":
        out, writes = c, False
    elif what == "out_is_stderr":
        out, writes = S, False
    elif what == "out_is_variance":
        var = out.reshape(-1)[8:24].reshape(4, 4)
    elif what == "variance_is_stderr":
        var, writes = S.reshape(-1)[48:64].reshape(4, 4), False
    elif what == "variance_is_normal":
        var, writes = nm.reshape(-1)[:16].reshape(4, 4), False
    elif what == "no_stderr":
        S = None
    elif what == "no_colour":
        c = None
    elif what == "nine_iterations":
        p.iterations = 9
    elif what == "sigma_zero":
        p.sigma_normal = 0.0
    elif what == "sigma_nan":
        p.sigma_colour = float("nan")
    elif what == "sigma_negative":
        p.sigma_albedo = -1.0
    elif what == "zero_width":
        w = 0
    elif what == "zero_height":
        h = 0
    elif what == "flags":
        p.flags = 1
    elif what.startswith("floor_"):
        floor = {"zero": 0.0, "negative": -1e-4, "nan": float("nan"), "inf": float("inf")}[what[6:]]
    rc, msg = _call(c, S, out, var, w, h, p, floor, nm)
    assert rc == N.IZPI_ERR_INVALID and msg == MESSAGES[what], (rc, msg)
    if writes:
        assert (out == 7.0).all() and (var == 7.0).all()  # nothing was written
    # the limits themselves are fine, and so is a call without a variance output
    rc, _ = _call(np.ones((4, 4, 4)), np.full((4, 4, 4), 0.1), np.zeros((4, 4, 4)), None, 4, 4,
                  N.denoise_params(8, float("inf"), float("inf"), float("inf")), 5e-324)
    assert rc == N.IZPI_OK


# ------------------------------------------------------------ 4. the entries
def test_entries_are_declared_exported_and_listed():
    L = N.lib()
    gpu_h = (ROOT / "include" / "izpi_gpu.h").read_text()
    host_h = (ROOT / "include" / "izpi_host.h").read_text()
    for name in NEW:
        assert name in N.EXPORTS and hasattr(L, name)
        assert ("int %s(" % name) in (host_h if name.startswith("izpi_host") else gpu_h)
    listed = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW:
        assert name in listed, name
    assert N.IZPI_ABI_VERSION == 4 and L.izpi_abi_struct_size(len(N.ABI_STRUCTS)) == 0  # no new struct


def test_a_null_context_is_invalid():
    L = N.lib()
    c, S = _flat(size=4)
    out, var = np.zeros_like(c), np.zeros((4, 4))
    for entry in (L.izpi_gpu_denoise_var, L.izpi_gpu_denoise_var_device):
        rc = entry(None, _p(c), _p(S), None, None, _p(out), _p(var), 4, 4, None, N.DENOISE_VAR_DEFAULT_FLOOR, None)
        assert rc == N.IZPI_ERR_INVALID
    assert (out == 0).all() and (var == 0).all()


# ------------------------------------------------------------ sanitizer program
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "denoise_var_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "denoise_var_check.cpp"),
                    str(CSRC / "denoise_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {ln.split()[1] for ln in lines if ln.startswith("case ")}
    assert ran >= {"40x30", "1x1", "1x7", "37x19", "64x64", "hand", "arguments"}, ran


# ------------------------------------------------------------ 5. it helps where the old filter hurts
@functools.lru_cache(maxsize=None)
def cornell_measurement():
    """configs.cornell_rgb at 48 x 48, seed 12345: 64 one-sample canvases from the oracle
    (tests/noise_ref.py), Normal / Albedo at 4 spp from the preview reference, the truth the
    oracle at 4096 spp with another seed; the mask is section 3.8's (written pixels whose truth
    is <= 1 in every channel). Rows: 16 spp, 64 spp, and an adaptive frame (threshold 0.25,
    steps of 16, cap 64: a pixel keeps the samples it had when its e fell to the threshold).
    Each row: RMSE of the frame, of host_denoise at its defaults, of host_denoise_var at its."""
    W = H = 48
    scene = configs.cornell_rgb()
    canvases = NR.sample_canvases(scene, W, H, 64, N.SAMPLER_COLOUR, N.ACC_FORWARD, seed=12345)
    o = O.OracleScene(scene, aspect_override=W / H)
    req = N.RenderReq(width=W, height=H, spp=4096, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=777,
                      abi_version=N.IZPI_ABI_VERSION, accumulation=N.ACC_FORWARD)
    truth = o.render(req, threads=16)[0].reshape(H, W, 4)
    o.close()
    ref = PR.PreviewRef(scene, W, H, 4)
    normal = ref.render(N.SAMPLER_NORMAL).reshape(H, W, 4)
    albedo = ref.render(N.SAMPLER_ALBEDO).reshape(H, W, 4)
    ref.close()
    mask = (truth[..., 3] != 0) & (truth[..., :3] <= 1.0).all(axis=2)

    def rmse(img):
        return float(np.sqrt(((img[..., :3] - truth[..., :3])[mask] ** 2).mean()))

    def frame(n):
        """(canvas, standard errors, e) after n samples of every pixel."""
        s, m2 = NR.fold(canvases, n)
        se, e, _ = NR.pixel_rule(s, m2, n, N.SAMPLER_COLOUR, N.NOISE_DEFAULT_FLOOR)
        c = np.zeros((H, W, 4))
        c[..., :3] = NR.mean_of(s, n, N.SAMPLER_COLOUR)
        c[..., 3] = canvases[0][..., 3]
        S = np.zeros((H, W, 4))
        S[..., :3] = se
        S[..., 3] = c[..., 3]
        S[c[..., 3] == 0] = 0.0
        return c, S, e

    frames = {n: frame(n) for n in (16, 32, 48, 64)}
    c, S = frames[16][0].copy(), frames[16][1].copy()
    n_map = np.full((H, W), 16)
    active = frames[16][2] > 0.25
    for n in (32, 48, 64):
        c[active], S[active], n_map[active] = frames[n][0][active], frames[n][1][active], n
        active = active & (frames[n][2] > 0.25)
    rows = {"16 spp": frames[16][:2], "64 spp": frames[64][:2], "adaptive": (c, S)}
    out = {}
    for name, (c, S) in rows.items():
        out[name] = (rmse(c), rmse(host_denoise(c, normal, albedo)), rmse(host_denoise_var(c, S, normal, albedo)[0]))
    return out, float(n_map[mask].mean()), sorted(set(n_map[mask].tolist()))


@pytest.mark.parametrize("row", ["16 spp", "64 spp", "adaptive"])
def test_it_beats_the_unfiltered_frame_and_the_fixed_sigma_filter(row):
    """Measured through the host twins at the defaults (sigma_colour 1.5, floor 1e-4, 5 iterations;
    RMSE unfiltered / section 3.8's filter / this one), the figures of DESIGN.md section 3.8a:
      16 spp    0.0804 / 0.0479 / 0.0399
      64 spp    0.0435 / 0.0487 / 0.0246
      adaptive  0.0613 / 0.0468 / 0.0331   (mean n 30.8 over n in {16, 32, 48, 64})"""
    rows, mean_n, ns = cornell_measurement()
    noisy, fixed, guided = rows[row]
    print("%s: unfiltered RMSE %.4f, izpi_host_denoise %.4f, izpi_host_denoise_var %.4f" % (row, noisy, fixed, guided))
    if row == "adaptive":
        print("adaptive: mean n %.1f over n in %s" % (mean_n, ns))
        assert len(ns) > 1
    assert guided < noisy
    assert guided < fixed
