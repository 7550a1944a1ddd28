"""The edge-avoiding a-trous denoiser without a GPU: the host twin
(izpi_host_denoise, izpi_amd/csrc/denoise_host.cpp) against the Python restatement
(tests/denoise_ref.py) to the byte, two properties that follow from the rule, the argument
checks, a stand-alone program under AddressSanitizer and UBSan, and a measured noise
reduction on a Cornell box against a 1024-sample truth."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.renderer import host_denoise
from oracle import oracle as O
from tests import denoise_ref as DR
from tests import preview_ref as PR

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"


# ------------------------------------------------------------ 1. twin == restatement
@pytest.mark.parametrize("case", DR.cases(), ids=DR.case_id)
def test_twin_equals_the_restatement_bytewise(case):
    w, h, variant, n, guides = case
    c, nm, al = DR.seeded(w, h, variant=variant)
    keep = c.copy()
    nm, al = DR.pick_guides(nm, al, guides)
    got = host_denoise(c, nm, al, N.denoise_params(iterations=n))
    want = DR.reference(case)
    assert got.tobytes() == want.tobytes(), "max |diff| %g" % np.nanmax(np.abs(got - want))
    assert c.tobytes() == keep.tobytes()  # the input is read only
    if n == 0:
        assert got.tobytes() == c.tobytes()
    elif w * h > 1:
        assert got.tobytes() != c.tobytes()  # it did something
    if variant == "dead_row0":
        assert got[0].tobytes() == c[0].tobytes()
    if variant in ("nan_pixel", "inf_pixel"):
        cy, cx = h // 2, w // 3
        assert got[cy, cx].tobytes() == c[cy, cx].tobytes()  # copied through, all four doubles
        mask = np.ones((h, w), bool)
        mask[cy, cx] = False
        assert np.isfinite(got[mask]).all()  # and it reached no neighbour
    if variant == "nan_guide":
        assert np.isfinite(got).all()


def test_null_params_are_the_defaults():
    c, nm, al = DR.seeded(37, 19)
    assert host_denoise(c, nm, al).tobytes() == host_denoise(c, nm, al, N.denoise_params(5, 1.0, 0.5, 0.5)).tobytes()
    assert (N.DENOISE_DEFAULT_ITERATIONS, N.DENOISE_MAX_ITERATIONS) == (5, 8)


# ------------------------------------------------------------ 2. variance, derivable
def test_one_iteration_without_edges_is_the_b3_kernel():
    """With no guides and sigma_colour 1e30 every weight is h*h: the output is the 5 x 5 B3
    kernel over the input, whose variance gain on white noise is (sum h^2)^2 = (35/128)^2,
    about 0.075. The bound is 0.25, three times that."""
    rng = np.random.default_rng(5)
    c = np.ones((32, 32, 4))
    c[..., :3] = 0.5 + rng.normal(0.0, 0.1, (32, 32, 3))
    got = host_denoise(c, params=N.denoise_params(1, sigma_colour=1e30))
    vin, vout = c[2:-2, 2:-2, :3].var(), got[2:-2, 2:-2, :3].var()
    print("variance in %.6f out %.6f ratio %.4f (B3: %.4f)" % (vin, vout, vout / vin, (35.0 / 128.0) ** 2))
    assert vout < 0.25 * vin


# ------------------------------------------------------------ 3. no leakage, exact
def test_a_normal_edge_stops_the_filter_exactly():
    """exp(-2e6) is 0, so a pixel only ever sums its own side, where every tap has the
    centre's colour: sc = sum(w) * colour accumulates the same addends as sw, times 1 or 0."""
    c = np.ones((24, 24, 4))
    c[:, 12:, :3] = 0.0
    nm = np.zeros((24, 24, 4))
    nm[:, :12, 0] = 1.0
    nm[:, 12:, 1] = 1.0
    got = host_denoise(c, nm, None, N.denoise_params(5, sigma_colour=1e30, sigma_normal=1e-3))
    assert got.tobytes() == c.tobytes()


# ------------------------------------------------------------ 4. argument checks
def _call(colour, out, w, h, params):
    L = N.lib()
    rc = L.izpi_host_denoise(colour.ctypes.data_as(C.c_void_p), None, None, out.ctypes.data_as(C.c_void_p), w, h,
                             None if params is None else C.byref(params))
    return rc, L.izpi_host_last_error().decode()


@pytest.mark.parametrize("what", ["alias", "nine_iterations", "sigma_zero", "sigma_nan", "sigma_negative", "zero_width",
                                  "zero_height", "flags"])
def test_bad_arguments_are_refused_with_a_message(what):
    c = np.ones((4, 4, 4))
    out = np.full((4, 4, 4), 7.0)
    p = N.denoise_params()
    w = h = 4
    if what == "alias":
        out = c
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
    rc, msg = _call(c, out, w, h, p)
    assert rc == N.IZPI_ERR_INVALID and msg.startswith("denoise: "), (rc, msg)
    if what != "alias":
        assert (out == 7.0).all()  # nothing was written
    rc, _ = _call(c, np.zeros((4, 4, 4)), 4, 4, N.denoise_params(8, float("inf"), float("inf"), float("inf")))
    assert rc == N.IZPI_OK  # the limits themselves are fine


# ------------------------------------------------------------ sanitizer program
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "denoise_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "denoise_check.cpp"),
                    str(CSRC / "denoise_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {ln.split()[1] for ln in lines if ln.startswith("case ")}
    assert ran >= {"40x30", "1x1", "1x7", "37x19", "64x64", "arguments"}, ran


# ------------------------------------------------------------ 5. it denoises
def test_it_denoises_a_cornell_box():
    """configs.cornell_rgb at 48 x 48, seed 12345: Colour from the oracle at 4 and 16 spp,
    Normal / Albedo at 4 spp from the preview reference, the truth the oracle at 1024 spp;
    RMSE over the written pixels whose truth is <= 1 in every channel (the few light-edge
    pixels otherwise carry most of any RMSE). Defaults, through the host twin. Measured
    with the scratch restatement the rule was chosen on: 0.43 x at 4 spp, 0.64 x at 16."""
    W = H = 48
    scene = configs.cornell_rgb()
    o = O.OracleScene(scene, aspect_override=W / H)

    def colour(spp):
        req = N.RenderReq(width=W, height=H, spp=spp, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345)
        return o.render(req, threads=16)[0].reshape(H, W, 4)

    truth = colour(1024)
    ref = PR.PreviewRef(scene, W, H, 4)
    normal = ref.render(N.SAMPLER_NORMAL).reshape(H, W, 4)
    albedo = ref.render(N.SAMPLER_ALBEDO).reshape(H, W, 4)
    ref.close()
    mask = (truth[..., 3] != 0) & (truth[..., :3] <= 1.0).all(axis=2)
    print("written pixels", int((truth[..., 3] != 0).sum()), "in the mask", int(mask.sum()))

    def rmse(img):
        return float(np.sqrt(((img[..., :3] - truth[..., :3])[mask] ** 2).mean()))

    ratios = {}
    for spp in (4, 16):
        noisy = colour(spp)
        den = host_denoise(noisy, normal, albedo)
        ratios[spp] = rmse(den) / rmse(noisy)
        print("%d spp: noisy RMSE %.4f denoised %.4f ratio %.3f" % (spp, rmse(noisy), rmse(den), ratios[spp]))
    o.close()
    assert ratios[4] < 0.75
    assert ratios[16] < 1.0
