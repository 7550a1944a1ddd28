"""The noise estimate of a progressive session without a GPU: the host
twin (izpi_host_noise, izpi_amd/csrc/noise_host.cpp) against the numpy restatement
(tests/noise_ref.py) to the byte on hand cases and on sums derived from the oracle, the
argument checks, the stop rule's boundary, a stand-alone program under AddressSanitizer and
UBSan, and the new entry points' declarations and NULL handling."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd.renderer import host_noise
from oracle import oracle as O
from tests import noise_ref as NR
from tests.test_abi import declared_functions

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"
INF, NAN = float("inf"), float("nan")


def check_against_ref(sums, m2, done, sampler, counted=None, **kw):
    """The twin's se and statistic equal the restatement's, byte for byte; returns both."""
    p = N.noise_params(**kw)
    se, st = host_noise(sums, m2, done, sampler, counted, p)
    rse, e, finite = NR.pixel_rule(np.reshape(sums, (-1, 3)), np.reshape(m2, (-1, 3)), done, sampler, p.floor)
    mask = np.ones(len(e), bool) if counted is None else np.asarray(counted, bool)
    ref = NR.frame_stat(e, finite, mask, done, p.threshold, p.tolerated, p.min_spp)
    assert se[:, :3].tobytes() == rse.tobytes()
    assert (se[:, 3] == 1.0).all()
    assert st["device_ms"] == 0.0
    for k, v in ref.items():
        if isinstance(v, float):
            assert np.float64(st[k]).tobytes() == np.float64(v).tobytes(), (k, st[k], v)
        else:
            assert st[k] == v, (k, st[k], v)
    return se, st, e


def folded(samples):
    """(sums, moment2) of samples (n, pixels, 3), folded in sample order."""
    s, m2 = np.zeros(samples.shape[1:]), np.zeros(samples.shape[1:])
    with np.errstate(all="ignore"):
        for x in samples:
            s = s + x
            m2 = m2 + x * x
    return s, m2


# ------------------------------------------------------------ 1. hand cases, exact
@pytest.mark.parametrize("sampler", [N.SAMPLER_COLOUR, N.SAMPLER_SPECTRAL])
def test_constant_samples_have_no_error(sampler):
    s, m2 = folded(np.full((4, 1, 3), 0.5))
    se, st, e = check_against_ref(s, m2, 4, sampler, min_spp=2)
    assert not se[:, :3].any() and e[0] == 0.0 and st["max_error"] == 0.0 and st["sum_error"] == 0.0
    assert (st["pixels"], st["above"], st["nonfinite"], st["converged"]) == (1, 0, 0, 1)


def test_zero_one_zero_one_has_variance_one_third():
    x = np.zeros((4, 1, 3))
    x[1] = x[3] = 1.0
    s, m2 = folded(x)
    se, st, e = check_against_ref(s, m2, 4, N.SAMPLER_COLOUR)
    v = (2.0 - (2.0 * 2.0) / 4.0) / 3.0
    assert v == 1.0 / 3.0
    assert se[0, 0] == np.sqrt(np.float64(v) / 4.0)
    assert e[0] == ((se[0, 0] + se[0, 1]) + se[0, 2]) / (((0.5 + 0.5) + 0.5) + 0.01)
    assert st["above"] == 1 and st["max_error"] == e[0] and st["sum_error"] == e[0]


def test_special_pixels():
    """A pixel whose s * s overflows (its variance goes to -Inf, so to 0: finite), a NaN sum,
    an Inf moment, and a plain one."""
    s = np.array([[2.4e154, 1.0, 1.0], [NAN, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    m2 = np.array([[1.44e308, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, INF, 1.0], [2.0, 2.0, 2.0]])
    with np.errstate(all="ignore"):
        assert np.isinf(s[0, 0] * s[0, 0]) and np.isfinite(m2[0, 0])
    se, st, e = check_against_ref(s, m2, 4, N.SAMPLER_COLOUR)
    assert se[0, 0] == 0.0 and np.isfinite(e[0])
    assert se[1, 0] == 0.0 and np.isnan(e[1])  # NaN variance -> 0; the mean carries the NaN
    assert np.isinf(se[2, 1])
    assert (st["pixels"], st["nonfinite"]) == (4, 2)
    assert st["max_error"] == max(e[0], e[3])


def test_two_samples():
    x = np.array([[[0.25, 0.5, 1.0]], [[0.75, 0.5, 3.0]]])
    s, m2 = folded(x)
    se, st, _ = check_against_ref(s, m2, 2, N.SAMPLER_SPECTRAL, min_spp=2)
    assert se[0, 0] == 0.25 and se[0, 1] == 0.0 and se[0, 2] == 1.0  # |a - b| / 2


# ------------------------------------------------------------ 2. the tree's blocks
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1200])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_block_sizes(n, masked):
    rng = np.random.default_rng(n)
    x = rng.random((5, n, 3)) * rng.random((1, n, 1)) * 4.0
    x[:, ::7] = 0.0  # black pixels
    s, m2 = folded(x)
    if n > 3:
        s[3, 1] = NAN
    counted = (np.arange(n) % 5 != 0) if masked else None
    _, st, e = check_against_ref(s, m2, 5, N.SAMPLER_COLOUR, counted, threshold=0.3)
    assert st["pixels"] == (int(counted.sum()) if masked else n)
    assert st["nonfinite"] == (1 if n > 3 else 0)
    if n == 1200:  # the blocking is part of the number: a plain left-to-right sum differs
        good = np.isfinite(e) & (counted if masked else True)
        plain = 0.0
        for v in e[good]:
            plain += v
        assert abs(st["sum_error"] - plain) <= n * 2.0 ** -53 * plain


# ------------------------------------------------------------ 3. arguments, the stop rule
def _call(params, done=4, sampler=N.SAMPLER_COLOUR, sums=True, m2=True):
    L = N.lib()
    a = np.ones(3)
    st = N.NoiseStats()
    rc = L.izpi_host_noise(a.ctypes.data_as(C.c_void_p) if sums else None, a.ctypes.data_as(C.c_void_p) if m2 else None, None,
                           1, done, sampler, None if params is None else C.byref(params), None, C.byref(st))
    return rc, L.izpi_host_last_error().decode(), st


@pytest.mark.parametrize("field, value", [("threshold", 0.0), ("threshold", -1.0), ("threshold", INF), ("threshold", NAN),
                                          ("floor", 0.0), ("floor", INF), ("floor", NAN), ("tolerated", -0.01),
                                          ("tolerated", 1.01), ("tolerated", NAN), ("flags", 1)])
def test_bad_parameters_are_refused_with_a_message(field, value):
    p = N.noise_params()
    setattr(p, field, value)
    rc, msg, st = _call(p)
    assert rc == N.IZPI_ERR_INVALID and msg.startswith("noise: "), (rc, msg)
    assert st.pixels == 0  # nothing was written


def test_other_argument_checks():
    for kw in ({"sums": False}, {"m2": False}, {"done": 0}, {"done": 1}, {"sampler": 0}, {"sampler": 6}):
        rc, msg, _ = _call(N.noise_params(), **kw)
        assert rc == N.IZPI_ERR_INVALID and msg.startswith("noise: "), (kw, rc, msg)
    for p in (None, N.noise_params(1e-300, 1e-300, 0.0, 0), N.noise_params(1e300, 1e300, 1.0, 2 ** 32 - 1)):
        assert _call(p)[0] == N.IZPI_OK  # NULL is the defaults; the limits themselves are fine


def test_null_params_are_the_defaults():
    rng = np.random.default_rng(3)
    s, m2 = folded(rng.random((8, 300, 3)))
    assert host_noise(s, m2, 8)[1] == host_noise(s, m2, 8, params=N.noise_params(0.25, 0.01, 0.05, 8))[1]


def test_converged_at_the_boundary():
    """20 pixels, 2 of them non-finite, 9 above: converged exactly when tolerated * 18 >= 9."""
    x = np.zeros((4, 20, 3))
    x[1, :9] = x[3, :9] = 1.0  # 9 noisy pixels (e = 0.57), 11 constant ones
    x[:, 9:] = 0.5
    s, m2 = folded(x)
    s[18, 0] = NAN
    m2[19, 2] = INF
    for tolerated, want in ((0.5, 1), (0.4999, 0), (1.0, 1), (0.0, 0)):
        _, st, _ = check_against_ref(s, m2, 4, N.SAMPLER_COLOUR, tolerated=tolerated, min_spp=4)
        assert (st["pixels"], st["nonfinite"], st["above"]) == (20, 2, 9)
        assert st["converged"] == want, tolerated
    _, st, _ = check_against_ref(s, m2, 4, N.SAMPLER_COLOUR, tolerated=0.5, min_spp=5)
    assert st["converged"] == 0  # done < min_spp


# ------------------------------------------------------------ 4. real data
@pytest.mark.parametrize("which, acc", [("cornell", N.ACC_RECURSIVE), ("cornell", N.ACC_FORWARD),
                                        ("special_spectral", N.ACC_FORWARD)])
def test_twin_on_oracle_sums(which, acc):
    size = (40, 30) if which == "cornell" else None
    canvases, W, H, sampler = NR.case_canvases(which, acc, 8, size)
    s, m2, counted = NR.packed_sums(canvases, 8, W, H)
    se, st, _ = check_against_ref(s, m2, 8, sampler, counted, threshold=0.25, tolerated=0.5, min_spp=4)
    snap, ref = NR.reference(canvases, 8, W, H, sampler, threshold=0.25, tolerated=0.5, min_spp=4)
    assert {k: st[k] for k in ref} == ref  # (NaN-free: the statistic holds finite numbers only)
    assert st["pixels"] == W * (H - 1)
    print(which, acc, st)
    if which == "special_spectral":
        assert st["nonfinite"] > 0  # the case with non-finite pixels: the branch is exercised
    else:
        assert st["nonfinite"] == 0 and 0 < st["above"] < st["pixels"]


def test_the_sample_canvases_fold_to_the_oracle_canvas():
    """What the reference rests on: the one-sample renders, summed in sample order and
    normalised by the canvas rule, are the oracle's canvas at spp = n, bit for bit."""
    from tests.test_forward_accumulation import scene_case
    for which, acc in (("cornell", N.ACC_FORWARD), ("special_spectral", N.ACC_FORWARD)):
        size = (40, 30) if which == "cornell" else None
        canvases, W, H, sampler = NR.case_canvases(which, acc, 8, size)
        o = O.OracleScene(scene_case(which)[0], aspect_override=W / H)
        for n in (3, 8):
            req = N.RenderReq(width=W, height=H, spp=n, max_depth=50, sampler=sampler, seed=12345,
                              abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
            want = o.render(req, threads=8)[0].reshape(H, W, 4)
            got = NR.mean_of(NR.fold(canvases, n)[0], n, sampler)
            assert got[1:].tobytes() == want[1:, :, :3].tobytes(), (which, n)
        o.close()


# ------------------------------------------------------------ sanitizer program
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "noise_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "noise_check.cpp"),
                    str(CSRC / "noise_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {" ".join(ln.split()[1:]) for ln in lines if ln.startswith("case ")}
    assert ran >= {"1 pixels", "255 pixels", "256 pixels", "257 pixels", "1200 pixels", "hand", "arguments"}, ran


# ------------------------------------------------------------ 5. the entry points
SINGLE = ["izpi_gpu_progressive_begin_ex", "izpi_gpu_progressive_noise", "izpi_gpu_progressive_converge"]
MULTI = ["izpi_gpu_multi_progressive_begin_ex", "izpi_gpu_multi_progressive_noise", "izpi_gpu_multi_progressive_converge"]


def test_entry_points_are_declared_exported_and_listed():
    L = N.lib()
    decl = declared_functions()
    for name in SINGLE + MULTI + ["izpi_host_noise"]:
        assert name in decl, name
        assert hasattr(L, name), name
        assert name in N.EXPORTS, name
    assert (N.SNAP_NOISE, N.PROG_NOISE) == (2, 1)
    assert N.NoiseParams in N.ABI_STRUCTS and N.NoiseStats in N.ABI_STRUCTS
    for i in (N.ABI_STRUCTS.index(N.NoiseParams), N.ABI_STRUCTS.index(N.NoiseStats)):
        assert L.izpi_abi_struct_size(i) == C.sizeof(N.ABI_STRUCTS[i])
    assert (C.sizeof(N.NoiseParams), C.sizeof(N.NoiseStats)) == (32, 56)


def test_null_context_is_invalid():
    L = N.lib()
    req = N.RenderReq(width=8, height=8, spp=2, sampler=N.SAMPLER_COLOUR, abi_version=N.IZPI_ABI_VERSION)
    st, ns, p = N.RenderStats(), N.NoiseStats(), N.noise_params()
    out = np.zeros(8 * 8 * 4)
    for pre in ("izpi_gpu_progressive_", "izpi_gpu_multi_progressive_"):
        assert getattr(L, pre + "begin_ex")(None, C.byref(req), 1, N.PROG_NOISE) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "noise")(None, C.byref(p), C.byref(ns)) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "noise")(None, None, None) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "converge")(None, C.byref(p), C.byref(st), C.byref(ns)) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "converge")(None, None, None, None) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "snapshot")(None, N.SNAP_NOISE, out.ctypes.data_as(C.c_void_p)) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_progressive_snapshot_device(None, N.SNAP_NOISE, None) == N.IZPI_ERR_INVALID
    assert not out.any() and ns.pixels == 0
