"""Adaptive sampling of a progressive session without a GPU: the host
twin (izpi_host_adapt, izpi_amd/csrc/noise_host.cpp) against the numpy restatement
(tests/adapt_ref.py) bit for bit over whole sessions, the reference's own active counts, the
argument checks, a stand-alone program under AddressSanitizer and UBSan, the new entry points
and structure, and the Python and command-line argument rules."""
import ctypes as C
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import build
from izpi_amd.renderer import ProgressiveSession, host_adapt
from tests import adapt_ref as AR
from tests.test_abi import declared_functions

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"
INF, NAN = float("inf"), float("nan")
RULE = dict(threshold=0.25, floor=0.01, tolerated=0.05, min_spp=4)
INTS = ("pixels", "nonfinite", "active", "retired", "samples", "done", "converged")


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, "not bit-identical: %d values differ, first %s" % (len(bad), bad[:5].tolist())


# ------------------------------------------------------------ 1. whole sessions against the reference
@pytest.mark.parametrize("which, size, steps, threshold, counts", [
    ("cornell", (40, 30), [4] * 8, 0.25, [716, 614, 502, 384, 285, 221, 184, 159]),
    ("cornell", (40, 30), [4] * 8, 0.5, None),
    ("glass_spectral", None, [4] * 4, 0.25, [493, 485, 471, 464]),
    ("special_spectral", None, [4] * 4, 0.25, None),
])
def test_twin_follows_the_reference(which, size, steps, threshold, counts):
    """Forward accumulation, seed 12345, adapt after every step: the twin's active set, e and
    integers are the reference's at every evaluation; the quoted counts are the reference's own."""
    rule = dict(RULE, threshold=threshold)
    ref, W, H, sampler = AR.simulate(which, N.ACC_FORWARD, steps, rule, size=size, counters=False)
    if counts is not None:
        assert [st["adapt"]["active"] for st in ref] == counts
    if (which, threshold) == ("cornell", 0.5):
        assert [st["adapt"]["active"] for st in ref][-2:] == [52, 44]
    active = np.ones(len(ref[0]["n"]), bool)
    p = N.noise_params(**rule)
    for st in ref:
        active, e, got = host_adapt(st["sums"], st["m2"], st["n"], active, st["done"], sampler, st["counted"], p)
        assert np.array_equal(active, st["active"])
        same_bits(e, st["e"])
        assert {k: got[k] for k in INTS} == st["adapt"], (st["done"], got, st["adapt"])
        assert got["device_ms"] == 0.0
    if which == "special_spectral":
        assert ref[0]["adapt"]["nonfinite"] > 0 and not (ref[0]["active"] & ~np.isfinite(ref[0]["e"])).any()
    else:
        assert len(set(ref[-1]["n"].tolist())) >= 3  # staggered: at least 3 distinct sample counts


def test_retirement_is_final_and_uncounted_pixels_retire():
    """Hand case: 4 pixels after 4 samples. A noisy pixel stays; a quiet one, an uncounted noisy
    one and a NaN one retire; a second call at a threshold below every e re-activates nothing."""
    x = np.zeros((4, 4, 3))
    x[1, (0, 2)] = x[3, (0, 2)] = 1.0  # pixels 0 and 2: 0, 1, 0, 1 (e = 0.57)
    x[:, 1] = 0.5                      # pixel 1: constant
    s, m2 = x.sum(0), (x * x).sum(0)
    s[3, 0] = NAN
    counted = np.array([1, 1, 0, 1], np.uint8)
    n = np.full(4, 4, np.uint32)
    active, e, st = host_adapt(s, m2, n, np.ones(4, bool), 4, counted=counted, params=N.noise_params(0.25, 0.01, 0.5, 4))
    assert active.tolist() == [True, False, False, False]
    assert {k: st[k] for k in INTS} == {"pixels": 3, "nonfinite": 1, "active": 1, "retired": 3, "samples": 16, "done": 4,
                                        "converged": 1}  # 1 <= 0.5 * (3 - 1)
    assert e[1] == 0.0 and np.isnan(e[3])
    again, _, st = host_adapt(s, m2, n, active, 4, counted=counted, params=N.noise_params(1e-9, 0.01, 0.0, 4))
    assert again.tolist() == active.tolist() and (st["active"], st["retired"], st["nonfinite"], st["converged"]) == (1, 0, 1, 0)
    # a retired pixel is read at its own count: pixel 1 retired at 4 samples, the session is at 8
    n2 = np.array([8, 4, 4, 4], np.uint32)
    _, e2, st = host_adapt(s * [[2], [1], [1], [1]], m2 * [[2], [1], [1], [1]], n2, active, 8, counted=counted,
                           params=N.noise_params(0.25, 0.01, 0.5, 4))
    assert st["samples"] == 20 and e2[1] == 0.0


# ------------------------------------------------------------ 2. arguments
def _call(params, done=4, sampler=N.SAMPLER_COLOUR, sums=True, m2=True, samples=True, active=True):
    L = N.lib()
    a = np.ones(3)
    n, act = np.full(1, done, np.uint32), np.ones(1, np.uint8)
    st = N.AdaptStats()
    ptr = lambda arr, on: arr.ctypes.data_as(C.c_void_p) if on else None
    rc = L.izpi_host_adapt(ptr(a, sums), ptr(a, m2), None, ptr(n, samples), ptr(act, active), 1, done, sampler,
                           None if params is None else C.byref(params), None, C.byref(st))
    return rc, L.izpi_host_last_error().decode(), st, act


@pytest.mark.parametrize("field, value, message", [
    ("threshold", 0.0, "noise: threshold must be finite and greater than 0"),
    ("threshold", INF, "noise: threshold must be finite and greater than 0"),
    ("threshold", NAN, "noise: threshold must be finite and greater than 0"),
    ("floor", 0.0, "noise: floor must be finite and greater than 0"),
    ("floor", NAN, "noise: floor must be finite and greater than 0"),
    ("tolerated", -0.01, "noise: tolerated must lie in [0, 1]"),
    ("tolerated", 1.01, "noise: tolerated must lie in [0, 1]"),
    ("flags", 1, "noise: flags must be 0")])
def test_bad_parameters_are_refused_with_check_params_messages(field, value, message):
    p = N.noise_params()
    setattr(p, field, value)
    rc, msg, st, act = _call(p)
    assert rc == N.IZPI_ERR_INVALID and msg == message, (rc, msg)
    assert st.pixels == 0 and act[0] == 1  # nothing was written
    ns = N.NoiseStats()  # ... the very message izpi_host_noise gives
    a = np.ones(3)
    assert N.lib().izpi_host_noise(a.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), None, 1, 4, N.SAMPLER_COLOUR,
                                   C.byref(p), None, C.byref(ns)) == N.IZPI_ERR_INVALID
    assert N.lib().izpi_host_last_error().decode() == message


def test_other_argument_checks():
    for kw in ({"sums": False}, {"m2": False}, {"samples": False}, {"active": False}, {"done": 0}, {"done": 1},
               {"sampler": 0}, {"sampler": N.SAMPLER_NORMAL}, {"sampler": N.SAMPLER_WIREFRAME}, {"sampler": 6}):
        rc, msg, st, _ = _call(N.noise_params(), **kw)
        assert rc == N.IZPI_ERR_INVALID and msg.startswith("adapt: "), (kw, rc, msg)
        assert st.pixels == 0
    assert _call(None)[0] == N.IZPI_OK  # NULL is the defaults
    L = N.lib()  # every output may be NULL
    a, n, act = np.full(3, 4.0), np.full(1, 4, np.uint32), np.ones(1, np.uint8)  # four samples of 1.0
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    assert L.izpi_host_adapt(vp(a), vp(a), None, vp(n), vp(act), 1, 4, N.SAMPLER_COLOUR, None, None, None) == N.IZPI_OK
    assert act[0] == 0  # constant samples: e = 0, retired
    assert L.izpi_host_adapt(vp(a), vp(a), None, vp(n), vp(act), 0, 4, N.SAMPLER_COLOUR, None, None, None) == N.IZPI_OK


def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "adapt_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "adapt_check.cpp"),
                    str(CSRC / "noise_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {" ".join(ln.split()[1:]) for ln in lines if ln.startswith("case ")}
    assert ran >= {"1 pixels", "63 pixels", "64 pixels", "257 pixels", "1200 pixels", "arguments"}, ran


# ------------------------------------------------------------ 3. the entry points
NEW = ["izpi_gpu_progressive_adapt", "izpi_gpu_multi_progressive_adapt", "izpi_host_adapt"]


def test_entry_points_are_declared_exported_and_listed():
    L = N.lib()
    decl = declared_functions()
    for name in NEW:
        assert name in decl, name
        assert hasattr(L, name), name
        assert name in N.EXPORTS, name
    assert (N.PROG_ADAPTIVE, N.SNAP_SAMPLES) == (4, 3)
    assert N.ABI_STRUCTS.index(N.AdaptStats) == 20
    assert L.izpi_abi_struct_size(20) == C.sizeof(N.AdaptStats) == 56
    assert L.izpi_abi_struct_size(21) == 0


def test_null_context_is_invalid():
    L = N.lib()
    st, p = N.AdaptStats(), N.noise_params()
    for name in NEW[:2]:
        assert getattr(L, name)(None, C.byref(p), C.byref(st)) == N.IZPI_ERR_INVALID
        assert getattr(L, name)(None, None, None) == N.IZPI_ERR_INVALID
    req = N.RenderReq(width=8, height=8, spp=2, sampler=N.SAMPLER_COLOUR, abi_version=N.IZPI_ABI_VERSION)
    for pre in ("izpi_gpu_progressive_", "izpi_gpu_multi_progressive_"):
        assert getattr(L, pre + "begin_ex")(None, C.byref(req), 1, N.PROG_NOISE | N.PROG_ADAPTIVE) == N.IZPI_ERR_INVALID
    assert st.pixels == 0


# ------------------------------------------------------------ 4. Python and command-line argument rules
def test_python_refuses_adaptive_without_noise():
    owner = SimpleNamespace(ctx=None)  # (refused before any call reaches the library)
    req = N.RenderReq(width=8, height=8, spp=2, sampler=N.SAMPLER_COLOUR, abi_version=N.IZPI_ABI_VERSION)
    with pytest.raises(ValueError, match="adaptive=True needs noise=True"):
        ProgressiveSession(owner, req, 1, noise=False, adaptive=True)
    with pytest.raises(ValueError, match="samples and active"):
        host_adapt(np.ones((2, 3)), np.ones((2, 3)), np.ones(1), np.ones(2), 4)


@pytest.mark.parametrize("args, message", [
    (["--adaptive"], "--adaptive needs --progressive and --noise-threshold"),
    (["--progressive", "4", "--adaptive"], "--adaptive needs --progressive and --noise-threshold"),
    (["--progressive", "4", "--noise-threshold", "0.25", "--samples-out", "n.pfm"], "--samples-out needs --adaptive"),
    (["--adaptive", "--noise-threshold", "0.25"], "--noise-threshold needs --progressive"),
])
def test_cli_argument_rules(args, message, tmp_path):
    run = subprocess.run([str(build.CLI), "--scene", str(tmp_path / "none.pbtxt")] + args, capture_output=True, text=True,
                         timeout=60)
    assert run.returncode != 0 and message in run.stderr, run.stderr
