"""The noise estimate of a progressive session on the GPU (izpi_gpu_progressive_begin_ex with
IZPI_PROG_NOISE, IZPI_SNAP_NOISE, izpi_gpu_progressive_noise / _converge).

The reference is tests/noise_ref.py: the oracle's one-sample renders folded in numpy, never
another GPU render. Everything is compared bit for bit except sum_error across share plans,
whose bound is derived where it is used.
"""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import build, configs
from izpi_amd.renderer import GPURenderer, MultiGPURenderer
from tests import noise_ref as NR
from tests import preview_ref as PR
from tests.test_forward_accumulation import scene_case
from tests.test_gpu_forward import assert_bitwise, oracle_both

pytestmark = pytest.mark.gpu

ACCS = [N.ACC_RECURSIVE, N.ACC_FORWARD]
RULE = dict(threshold=0.25, floor=0.01, tolerated=0.5, min_spp=4)  # the stop-rule case's, used throughout
COUNTERS = ("rays", "node_visits", "tri_tests", "sph_tests", "light_tri_tests", "light_sph_tests", "samples")


def same_bits(got, want):
    """Bit-identical arrays (a NaN matches a NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, "not bit-identical: %d values differ, first %s" % (len(bad), bad[:5].tolist())


def same_stats(got, want):
    """Every field of the statistic but device_ms, the doubles by their bits."""
    for k, v in want.items():
        if isinstance(v, float):
            assert np.float64(got[k]).tobytes() == np.float64(v).tobytes(), (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)
    assert got["device_ms"] >= 0


def check_session(s, canvases, W, H, sampler, tiles=None):
    """The NOISE snapshot and the statistic of session s against the reference at s.done."""
    snap, stat = NR.reference(canvases, s.done, W, H, sampler, tiles, **RULE)
    same_bits(s.snapshot(N.SNAP_NOISE), snap)
    got = s.noise(**RULE)
    print("done", s.done, {k: got[k] for k in stat})
    same_stats(got, stat)
    return stat


def renderer(which, acc, size=None, **kw):
    scene, W, H, spp, sampler = scene_case(which)
    if size is not None:
        W, H = size
    return GPURenderer(scene, W, H, spp, sampler=sampler, accumulation=acc, **kw)


# ---- 1. every path of the fold
@pytest.mark.parametrize("acc", ACCS)
def test_every_path_of_the_fold(gpu, acc):
    """cornell at 40 x 30: 1200 pixels are four full 256-blocks and a partial one, so the
    LDS-staged form and the fallback run in one launch. step_spp 4, steps 1, 2, 4, 1: odd, even
    and multiple-of-4 chunks at s0 = 0, 1, 3, 7. Then one step of 8 on a workspace sized for 3."""
    canvases, W, H, sampler = NR.case_canvases("cornell", acc, 8, (40, 30))
    r = renderer("cornell", acc, (W, H))
    with r.progressive(4, noise=True) as s:
        for n in (1, 2, 4, 1):
            s.step(n)
            if s.done >= 2:
                stat = check_session(s, canvases, W, H, sampler)
                assert stat["pixels"] == W * (H - 1) and stat["nonfinite"] == 0 and stat["above"] > 0
        assert s.done == 8
    with r.progressive(3, noise=True) as s:
        s.step(8)
        assert s.done == 8 and s.stats["chunk_spp"] <= 3
        check_session(s, canvases, W, H, sampler)
    r.close()


# ---- 2. raw forward Spectral samples, non-finite pixels
@pytest.mark.parametrize("which", ["glass_spectral", "special_spectral"])
def test_spectral_scenes(gpu, which):
    """32 x 32, N = 8, forward accumulation: the samples are weighed (spectral_weigh) by the
    fold itself. special_spectral has non-finite pixels: as many as the reference counts."""
    canvases, W, H, sampler = NR.case_canvases(which, N.ACC_FORWARD, 8)
    r = renderer(which, N.ACC_FORWARD)
    with r.progressive(3, noise=True) as s:
        for _ in range(3):
            s.step()
            stat = check_session(s, canvases, W, H, sampler)
        assert s.done == 8
        if which == "special_spectral":
            assert stat["nonfinite"] > 0
    r.close()


# ---- 3. the flag changes no existing output
@pytest.mark.parametrize("acc", ACCS)
def test_the_existing_outputs_do_not_change(gpu, acc):
    which = "glass_spectral"
    scene, W, H, _, sampler = scene_case(which)
    r = renderer(which, acc)
    seen = {}
    for noise in (False, True):
        with r.progressive(3, noise=noise) as s:
            for _ in range(3):
                s.step()
                seen[noise, s.done] = (s.snapshot(), s.snapshot(N.SNAP_DISPLAY), {k: s.stats[k] for k in COUNTERS})
                if noise:
                    s.noise(**RULE)  # (neither the statistic nor the NOISE snapshot touches the sums)
                    s.snapshot(N.SNAP_NOISE)
    for done in (3, 6, 8):
        plain, flagged = seen[False, done], seen[True, done]
        assert flagged[0].tobytes() == plain[0].tobytes() and flagged[1].tobytes() == plain[1].tobytes()
        assert flagged[2] == plain[2]
    ref, ref_stats = oracle_both(scene, W, H, 8, sampler)[acc]
    assert_bitwise(seen[True, 8][0], ref, seen[True, 8][2], ref_stats)
    r.close()


# ---- 4. tiles and the packed layout
def test_tiles_packed(gpu):
    """Two 16 x 16 tiles packed, steps 2 and 2: tile after tile, each by sample row y then x."""
    acc = N.ACC_RECURSIVE
    canvases, W, H, sampler = NR.case_canvases("cornell", acc, 8)
    tiles = np.array(((0, 1, 15, 16), (16, 16, 31, 31)), np.uint32)
    r = renderer("cornell", acc)
    with r.progressive(2, total=4, tiles=tiles, layout=N.OUT_PACKED, noise=True) as s:
        for done in (2, 4):
            s.step()
            snap, stat = NR.reference(canvases, done, W, H, sampler, tiles, **RULE)
            want = np.concatenate([snap[H - y, x0:x1 + 1] for x0, y0, x1, y1 in tiles.tolist() for y in range(y0, y1 + 1)])
            got = s.snapshot(N.SNAP_NOISE)
            assert got.shape == (2 * 16 * 16 * 4,)
            same_bits(got.reshape(-1, 4), want)
            same_stats(s.noise(**RULE), stat)
            assert stat["pixels"] == 512
    r.close()


# ---- 5. a preview sampler
PAPER, INK = (0.1, 0.2, 0.3), (1.0, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def wireframe_canvases():
    """The WireFrame samples of cornell_rgb 32 x 32 x 4 from tests/preview_ref.py, as one canvas
    per sample (DeNAN applied, as rgb.go:36 adds them)."""
    W = H = 32
    ref = PR.PreviewRef(configs.cornell_rgb(), W, H, 4)
    samples = ref.wireframe_samples(PAPER, INK)[0]
    ref.close()
    out = [np.zeros((H, W, 4)) for _ in range(4)]
    k = 0
    for y in range(H):
        for x in range(W):
            for s in range(4):
                if y >= 1:
                    out[s][H - y, x] = PR.denan(samples[k]) + (1.0,)
                k += 1
    return out


def test_wireframe_sampler(gpu):
    W = H = 32
    r = GPURenderer(configs.cornell_rgb(), W, H, 4, sampler=N.SAMPLER_WIREFRAME, background=PAPER, ink=INK, bvh="gpu")
    with r.progressive(3, noise=True) as s:
        for n in (2, 2):
            s.step(n)
            stat = check_session(s, wireframe_canvases(), W, H, N.SAMPLER_WIREFRAME)
        assert 0 < stat["above"] < stat["pixels"]  # edges through some pixels, flat paper in others
    r.close()


# ---- 6. the rules
def test_rules(gpu):
    acc = N.ACC_FORWARD
    canvases, W, H, sampler = NR.case_canvases("cornell", acc, 8, (40, 30))
    L = N.lib()
    r = renderer("cornell", acc, (W, H))
    out = np.zeros((H, W, 4))
    ptr = out.ctypes.data_as(C.c_void_p)
    ns, good = N.NoiseStats(), N.noise_params(**RULE)
    req = r.request()
    for flags in (2, 3, 0x80000000):  # unknown begin flags
        assert L.izpi_gpu_progressive_begin_ex(r.ctx, C.byref(req), 4, flags) == N.IZPI_ERR_INVALID
    with r.progressive(4) as s:  # without the flag
        s.step(4)
        assert L.izpi_gpu_progressive_snapshot(r.ctx, N.SNAP_NOISE, ptr) == N.IZPI_ERR_INVALID
        assert b"IZPI_PROG_NOISE" in L.izpi_gpu_last_error(r.ctx)
        assert L.izpi_gpu_progressive_noise(r.ctx, C.byref(good), C.byref(ns)) == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_progressive_converge(r.ctx, C.byref(good), None, C.byref(ns)) == N.IZPI_ERR_INVALID
        assert s.snapshot().any()  # the session is intact
    assert L.izpi_gpu_progressive_noise(r.ctx, C.byref(good), C.byref(ns)) == N.IZPI_ERR_INVALID  # no session
    s = r.progressive(4, noise=True)
    for done in (0, 1):
        if done:
            s.step(1)
        assert L.izpi_gpu_progressive_snapshot(r.ctx, N.SNAP_NOISE, ptr) == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_progressive_noise(r.ctx, C.byref(good), C.byref(ns)) == N.IZPI_ERR_INVALID
    s.step(1)
    for field, value in (("threshold", 0.0), ("threshold", float("inf")), ("floor", float("nan")), ("floor", -1.0),
                         ("tolerated", 1.5), ("tolerated", -0.5), ("flags", 1)):
        bad = N.noise_params(**RULE)
        setattr(bad, field, value)
        assert L.izpi_gpu_progressive_noise(r.ctx, C.byref(bad), C.byref(ns)) == N.IZPI_ERR_INVALID, field
        assert L.izpi_gpu_last_error(r.ctx).startswith(b"noise: ")
        assert L.izpi_gpu_progressive_converge(r.ctx, C.byref(bad), None, None) == N.IZPI_ERR_INVALID, field
    assert not out.any() and ns.pixels == 0 and s.done == 2
    # the refusals of a plain session hold as they are
    st = N.RenderStats()
    assert L.izpi_gpu_progressive_begin_ex(r.ctx, C.byref(req), 4, N.PROG_NOISE) == N.IZPI_ERR_INVALID  # a second begin
    assert L.izpi_gpu_render(r.ctx, C.byref(req), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)) == N.IZPI_ERR_INVALID
    assert b"progressive session" in L.izpi_gpu_last_error(r.ctx)
    assert L.izpi_gpu_prepare(r.ctx, C.byref(req)) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_upload_scene(r.ctx, C.byref(r.host.desc)) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_progressive_snapshot(r.ctx, 7, ptr) == N.IZPI_ERR_INVALID
    # ... and left the session intact
    check_session(s, canvases, W, H, sampler)
    s.step(6)
    check_session(s, canvases, W, H, sampler)
    s.close()
    ref, ref_stats = oracle_both(scene_case("cornell")[0], W, H, 8, sampler)[acc]
    assert_bitwise(r.render(), ref, r.stats, ref_stats)  # a one-shot render after a noise session
    r.close()


# ---- 7. the stop rule
STOP = dict(which="cornell", acc=N.ACC_FORWARD, step=4, cap=32)


@functools.lru_cache(maxsize=None)
def stop_reference():
    """(sample canvases, W, H, sampler, the done at which the reference stops, its statistic)."""
    canvases, W, H, sampler = NR.case_canvases(STOP["which"], STOP["acc"], STOP["cap"])
    for done in range(STOP["step"], STOP["cap"] + 1, STOP["step"]):
        if done < max(2, RULE["min_spp"]):
            continue
        stat = NR.reference(canvases, done, W, H, sampler, **RULE)[1]
        print("reference: done %d above %d of %d" % (done, stat["above"], stat["pixels"] - stat["nonfinite"]))
        if stat["converged"]:
            return canvases, W, H, sampler, done, stat
    return canvases, W, H, sampler, STOP["cap"], stat


def test_the_stop_rule(gpu):
    """cornell 40 x 40, forward, seed 12345, steps of 4 up to 32, threshold 0.25, tolerated 0.5,
    min_spp 4. The reference stops strictly between the first evaluation and the cap (a
    condition on the inputs); the GPU stops at the same done with the oracle's canvas."""
    canvases, W, H, sampler, stop, stat = stop_reference()
    assert STOP["step"] < stop < STOP["cap"], stop
    scene = scene_case(STOP["which"])[0]
    r = GPURenderer(scene, W, H, STOP["cap"], sampler=sampler, accumulation=STOP["acc"])
    with r.progressive(STOP["step"], noise=True) as s:
        got = s.converge(**RULE)
        assert s.done == stop and got["done"] == stop and got["converged"] == 1
        same_stats(got, stat)
        canvas, counters = s.snapshot(), s.stats
    ref, ref_stats = oracle_both(scene, W, H, stop, sampler)[STOP["acc"]]
    assert_bitwise(canvas, ref, counters, ref_stats)
    img, last = r.render_until(RULE["threshold"], STOP["step"], floor=RULE["floor"], tolerated=RULE["tolerated"],
                               min_spp=RULE["min_spp"])
    assert last["done"] == stop and img.tobytes() == canvas.tobytes()
    cap = stop - STOP["step"]  # a cap below the stop: it ends there, not converged
    with r.progressive(STOP["step"], total=cap, noise=True) as s:
        got = s.converge(**RULE)
        assert s.done == cap and got["done"] == cap and got["converged"] == 0
    r.close()


# ---- 8. multi-GPU
@pytest.mark.parametrize("contexts", [2, 3])
def test_multi(gpu, contexts):
    """The integers, the maximum, the NOISE snapshot and the stopping done are one context's.
    sum_error adds the same non-negative terms in another order: each of the at most `pixels`
    additions rounds by at most 2^-53 relative to a partial sum that is at most the total, so
    two orders differ by at most pixels * 2^-53 relative (a bound, not a measurement)."""
    canvases, W, H, sampler, stop, stat = stop_reference()
    scene = scene_case(STOP["which"])[0]
    m = MultiGPURenderer(scene, W, H, STOP["cap"], [0] * contexts, sampler=sampler, bvh="reference", accumulation=STOP["acc"])
    with m.progressive(STOP["step"], noise=True) as s:
        s.step()
        snap, first = NR.reference(canvases, STOP["step"], W, H, sampler, **RULE)
        same_bits(s.snapshot(N.SNAP_NOISE), snap)
        for want in (first, None):
            if want is None:
                got, want = s.converge(**RULE), stat
                assert s.done == stop
            else:
                got = s.noise(**RULE)
            print(contexts, "contexts:", got)
            same_stats(got, {k: v for k, v in want.items() if k != "sum_error"})
            assert abs(got["sum_error"] - want["sum_error"]) <= want["pixels"] * 2.0 ** -53 * want["sum_error"]
        same_bits(s.snapshot(N.SNAP_NOISE), NR.reference(canvases, stop, W, H, sampler, **RULE)[0])
        canvas = s.snapshot()
    ref = oracle_both(scene, W, H, stop, sampler)[STOP["acc"]][0]
    assert canvas.tobytes() == ref.tobytes()
    L = N.lib()
    with m.progressive(STOP["step"]) as s:  # without the flag
        s.step()
        assert L.izpi_gpu_multi_progressive_noise(m.m, None, C.byref(N.NoiseStats())) == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_multi_progressive_snapshot(m.m, N.SNAP_NOISE, canvas.ctypes.data_as(C.c_void_p)) == N.IZPI_ERR_INVALID
    m.close()


# ---- 9. the command-line tool
def test_cli_stops_by_the_rule(gpu, tmp_path):
    """--progressive 4 --noise-threshold 0.25 on the RGB box: one IZPI_NOISE line per
    evaluation, --out is the one-shot's file at the printed done to the byte, --noise-out the
    NOISE snapshot of a session at that done."""
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(1.0))
    base = [str(build.CLI), "--scene", str(box), "--x", "40", "--y", "40"]
    out, se, one = tmp_path / "out.pfm", tmp_path / "se.pfm", tmp_path / "one.pfm"
    run = subprocess.run(base + ["--samples", "32", "--progressive", "4", "--noise-threshold", "0.25", "--noise-tolerated", "0.5",
                                 "--min-samples", "4", "--out", str(out), "--noise-out", str(se)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = [ln for ln in run.stderr.splitlines() if ln.startswith("IZPI_NOISE ")]
    fields = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines]
    assert all(sorted(f) == ["above", "done", "max", "mean", "nonfinite", "pixels"] for f in fields), lines
    dones = [int(f["done"]) for f in fields]
    done = dones[-1]
    assert dones == list(range(4, done + 1, 4)) and 4 < done < 32, lines
    assert int(fields[-1]["above"]) <= 0.5 * (int(fields[-1]["pixels"]) - int(fields[-1]["nonfinite"]))
    assert re.search(r'"spp": %d,' % done, run.stdout), run.stdout
    run = subprocess.run(base + ["--samples", str(done), "--out", str(one)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert out.read_bytes() == one.read_bytes()
    r = GPURenderer(configs.cornell_rgb(), 40, 40, 32, bvh="gpu", accumulation=N.ACC_FORWARD)
    with r.progressive(4, noise=True) as s:
        s.step(done)
        want = s.snapshot(N.SNAP_NOISE)
        stat = s.noise(**RULE)
    r.close()
    assert (int(fields[-1]["above"]), int(fields[-1]["pixels"])) == (stat["above"], stat["pixels"])
    head = b"PF\n40 40\n-1.0\n"
    data = se.read_bytes()
    assert data.startswith(head)
    pixels = np.frombuffer(data[len(head):], "<f4").reshape(40, 40, 3)[::-1]  # bottom row first
    assert np.array_equal(pixels, want[..., :3].astype(np.float32))
    run = subprocess.run(base + ["--noise-threshold", "0.25"], capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "--noise-threshold needs --progressive" in run.stderr
